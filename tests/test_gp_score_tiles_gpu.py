"""The resident scoring kernel's cross-tile path: batches in which every workgroup
loops over two or three 16-candidate tiles and the last tile is ragged.

Between tiles ``gp_score_kernel`` keeps two barriers: the waves that do not write the
(mu_n, q) rows run ahead into the next tile's phase 1 while the finishing wave still
reads the reduction buffer, the next tile's candidates are staged into ``cs`` during
phase 2, and the mu partials alternate between two halves of ``red`` by tile parity.
The other parity tests score 333 candidates (one tile per workgroup) and never get
there.  Checked per model:

  * mu and sd on 2048 sampled rows (first, middle and last tiles) against
    ``posterior_exact`` at the 1e-9 bars and scales of tests/test_gp_gpu.py, and the
    EI argmin of the whole batch against an fp64 host evaluation of the same
    triangular form when the oracle's top-2 gap exceeds 1e-9 relative;
  * position independence: the same rows scored again in chunks of one tile per
    workgroup (no second tile, so no run-ahead) give bit-equal mu -- the shares of
    the observations move round the waves from tile to tile, but their mu partials
    are folded in share order whichever wave computed them -- and sd^2 within
    8 eps amp y_std^2 (the q partials are summed in wave order, and which wave holds
    which columns depends on ``blockIdx.x & 3``);
  * the full batch scored twice gives identical outputs, top-k included.

The length scales (2..4) keep |x / ls|^2 <= 2 on [0, 1]^d, so the models with
d + 2 <= dp run phase 1 in its MFMA-distance form; (40, 12) has no spare columns and
runs the direct form, and the "far" case moves one tile in seven outside the bound so
that both forms alternate inside one workgroup's loop."""
import functools

import numpy as np
import pytest
import torch

from mpi_opt_amd._lib import MpoError
from oracle import gp_ei as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
AMP, NOISE = 2.0, 0.05


def _grid_bound():
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _problem(n, d, far):
    """Model, candidates and host references of one case (shared, read-only)."""
    G = _grid_bound()
    m = 16 * G * 2 + 16 * (G // 8) + 5
    X, y = O.synthetic_problem(n, d, seed=n + d)
    ls = np.linspace(2.0, 4.0, d)
    st = O.gp_from_theta(X, y, AMP, ls, NOISE)
    C = O.synthetic_candidates(m, d, seed=7)
    cc_max = float(np.sum(1.0 / ls ** 2))
    assert cc_max <= 2.0                                 # every unit-cube tile is inside the bound
    if far:
        C = C.copy()
        tiles = np.arange(3, (m + 15) // 16, 7)
        for t in tiles:
            C[16 * t:16 * t + 16] = C[16 * t:16 * t + 16] * 6.0 - 2.5
        cc = np.array([np.max(np.sum((C[16 * t:16 * t + 16] / ls) ** 2, axis=1)) for t in tiles])
        assert np.all(cc > 2.0)                          # each of them takes the direct form
    third = 2048 // 3
    mid = (m // 2) // 16 * 16
    sel = np.concatenate([np.arange(third), np.arange(mid, mid + third), np.arange(m - (2048 - 2 * third), m)])
    mu_x, sd_x = O.posterior_exact(st, C[sel])
    Ks = np.abs(O.matern52(C[sel], st.X, st.length_scale, st.amp))
    scale = st.y_std * (Ks @ np.abs(st.alpha)) + abs(st.y_mean)
    # whole batch in fp64, sd^2 = amp - ||L^-1 k||^2 (no cancellation inside the form)
    W = np.linalg.inv(st.L)
    vals = []
    for s in range(0, m, 16384):
        K = O.matern52(C[s:s + 16384], st.X, st.length_scale, st.amp)
        var = np.maximum(st.amp - np.sum((K @ W.T) ** 2, axis=1), 0.0)
        vals.append(O.acquisition_values(st.y_std * (K @ st.alpha) + st.y_mean, np.sqrt(var) * st.y_std,
                                         float(np.min(y)), "EI"))
    vals = np.concatenate(vals)
    for a in (C, sel, vals):
        a.setflags(write=False)
    return dict(X=X, y=y, st=st, C=C, sel=sel, mu_x=mu_x.astype(np.float64), sd_x=sd_x.astype(np.float64),
                scale=scale, ei=vals, y_opt=float(np.min(y)))


def _check(n, d, far=False, md=None):
    from mpi_opt_amd.gp import DeviceGP

    p = _problem(n, d, far)
    st, sel = p["st"], p["sel"]
    g = DeviceGP(p["X"], p["y"], st.amp, st.length_scale, st.noise)
    assert g.score_path == 0                             # the resident kernel
    if md is not None:
        assert bool(g.model.xb) == md
    C = torch.tensor(p["C"], device="cuda")
    m = C.shape[0]
    out = g.score(C, p["y_opt"], acqs=("EI",), k=5)
    torch.cuda.synchronize()
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()

    # oracle
    e_mu = np.max(np.abs(mu[sel] - p["mu_x"]) / p["scale"])
    e_sd = np.max(np.abs(sd[sel] - p["sd_x"]) / np.maximum(p["sd_x"], 1e-300))
    print(f"n={n} d={d} far={far} m={m}: mu err {e_mu:.3e}  sd err {e_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9
    srt = np.sort(p["ei"])
    if (srt[1] - srt[0]) > 1e-9 * abs(srt[0]) + 1e-300:
        assert int(out["topk"]["EI"][0][0]) == int(np.argmin(p["ei"]))

    # position independence: one tile per workgroup
    chunk = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    assert chunk <= 16 * _grid_bound()
    mu_c, sd_c = [], []
    for s in range(0, m, chunk):
        o = g.score(C[s:s + chunk], p["y_opt"], acqs=("EI",), k=5)
        mu_c.append(o["mu"])
        sd_c.append(o["sd"])
    mu_c, sd_c = torch.cat(mu_c), torch.cat(sd_c)
    dvar = float(torch.max(torch.abs(out["sd"] ** 2 - sd_c ** 2)))
    bad = int(torch.count_nonzero(out["mu"] != mu_c))
    print(f"  chunked: mu rows differing {bad}  max |dvar| {dvar:.3e} = {dvar / (EPS * st.amp * st.y_std ** 2):.2f} eps amp y_std^2")
    assert torch.equal(out["mu"], mu_c)
    assert dvar <= 8 * EPS * st.amp * st.y_std ** 2

    # repeat
    again = g.score(C, p["y_opt"], acqs=("EI",), k=5)
    assert torch.equal(out["mu"], again["mu"]) and torch.equal(out["sd"], again["sd"])
    assert torch.equal(out["values"]["EI"], again["values"]["EI"])
    assert torch.equal(out["topk"]["EI"][0], again["topk"]["EI"][0])
    assert torch.equal(out["topk"]["EI"][1], again["topk"]["EI"][1])


@pytest.mark.parametrize("n,d,md", [(16, 10, True), (40, 10, True), (200, 10, True), (40, 12, False), (40, 4, False)])
def test_looped_tiles(n, d, md):
    """(16, 10): one observation block, three waves idle in phase 1; (40, 10): three;
    (200, 10): the flagship's 4/3/3/3 split; (40, 12) and (40, 4): dp = d, no spare
    columns, so the direct form (EPT = 1 and a quarter-filled tile of threads)."""
    _check(n, d, md=md)


def test_far_tiles_alternate_distance_forms():
    _check(40, 10, far=True, md=True)


@pytest.mark.parametrize("occ", ["4", "6"])
def test_looped_tiles_forced_occupancy(occ, monkeypatch):
    monkeypatch.setenv("MPO_GP_OCC", occ)
    try:
        _check(40, 10)
    except MpoError as e:
        assert "invalid device function" in str(e).lower() or "hipErrorInvalidDeviceFunction" in str(e)
        pytest.skip(f"occupancy {occ} would spill: refused")
