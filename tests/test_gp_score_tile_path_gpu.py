"""The resident scoring kernel's per-tile path: phase 1's operand prefetch in the
MFMA-distance loop, the DPP column folds of mu and q, and the clamp of the MFMA
distance.

In the MFMA-distance form a wave's share of the 16-observation blocks is t = share,
share + 4, ...; block t + 4's ``xb`` fragments and alpha are loaded (asm loads, explicit
waits) while block t's Matern runs, the last block's prefetch re-reads that block, and
the loop drains before the mu fold.  What can go wrong there: a share of zero or one
blocks, a register consumed before its load landed or after the next load was issued
(a value that depends on where the row sits in the batch), a load still in flight when
the same wave takes the direct form for the next tile.

Bars: the project's own (tests/test_gp_gpu.py) -- mu (relative to its summand scale)
and sd against the oracle's extended-precision posterior within 1e-9, the MFMA
distance against the direct one within 1e-10, the top-5 identical between the two
forms; against an fp64 host evaluation of EI the top-5 is compared when the host's
own six lowest values are further apart than 1e-9 relative (closer than that the
host's order is not a reference).  Length scales are >= sqrt(d), so |x / ls|^2 <= 1 on
the unit cube and every such tile takes the expanded distance where the model has it
(d + 2 <= dp: d = 5 and 10 here; d = 2, 14 and 30 have no spare columns and run the
direct form through the same folds)."""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_ei as O

pytestmark = pytest.mark.gpu

AMP, NOISE = 2.0, 0.05


def _ls(d):
    return np.linspace(1.0, 1.5, d) * np.sqrt(d)


def _mu_scale(st, C):
    return st.y_std * (np.abs(O.matern52(C, st.X, st.length_scale, st.amp)) @ np.abs(st.alpha)) + abs(st.y_mean)


def _ei_host(st, C, y_opt):
    """EI of every row in fp64, sd^2 = amp - ||L^-1 k||^2."""
    W = np.linalg.inv(st.L)
    out = []
    for s in range(0, C.shape[0], 16384):
        K = O.matern52(C[s:s + 16384], st.X, st.length_scale, st.amp)
        var = np.maximum(st.amp - np.sum((K @ W.T) ** 2, axis=1), 0.0)
        out.append(O.acquisition_values(st.y_std * (K @ st.alpha) + st.y_mean, np.sqrt(var) * st.y_std, y_opt, "EI"))
    return np.concatenate(out)


def _score_both(p, monkeypatch):
    """{mode: (model, outputs)}: MPO_GP_DIST=1 (the MFMA distance where the model has it) and 0 (direct)."""
    from mpi_opt_amd.gp import DeviceGP

    st = p["st"]
    C = torch.tensor(p["C"], device="cuda")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPO_GP_DIST", mode)
        g = DeviceGP(p["X"], p["y"], st.amp, st.length_scale, st.noise)
        assert g.score_path == 0                         # the resident kernel
        out[mode] = (g, g.score(C, p["y_opt"], acqs=("EI",), k=5))
    torch.cuda.synchronize()
    return out


def _check_parity(p, out, label):
    st, sel = p["st"], p["sel"]
    (g0, o0), (g1, o1) = out["0"], out["1"]
    assert not g0.model.xb
    assert bool(g1.model.xb) == (g1.model.d + 2 <= g1.model.dp)
    mu0, sd0 = o0["mu"].cpu().numpy(), o0["sd"].cpu().numpy()
    mu1, sd1 = o1["mu"].cpu().numpy(), o1["sd"].cpu().numpy()
    e_mu = np.max(np.abs(mu1[sel] - p["mu_x"]) / p["scale"])
    e_sd = np.max(np.abs(sd1[sel] - p["sd_x"]) / p["sd_x"])
    full_scale = p["scale"] if len(sel) == len(mu1) else _mu_scale(st, p["C"])
    d_mu = np.max(np.abs(mu1 - mu0) / full_scale)
    d_sd = np.max(np.abs(sd1 - sd0) / sd0)
    print(f"{label}: mu err {e_mu:.3e}  sd err {e_sd:.3e}  md vs direct: mu {d_mu:.3e}  sd {d_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9
    assert d_mu < 1e-10
    assert d_sd < 1e-10
    top1 = o1["topk"]["EI"][0].cpu().numpy()
    assert np.array_equal(o0["topk"]["EI"][0].cpu().numpy(), top1)
    low = np.sort(p["ei"])[:6]
    if np.all(np.diff(low) > 1e-9 * np.abs(low[:-1]) + 1e-300):
        np.testing.assert_array_equal(top1, O.topk_lowest(p["ei"], 5))
    v1 = o1["values"]["EI"].cpu().numpy()
    np.testing.assert_allclose(v1, O.acquisition_values(mu1, sd1, p["y_opt"], "EI"), rtol=1e-10, atol=1e-300)


@functools.lru_cache(maxsize=None)
def _edge_problem(n, d):
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, AMP, _ls(d), NOISE)
    C = O.synthetic_candidates(1000, d, seed=11)
    mu_x, sd_x = O.posterior_exact(st, C)
    y_opt = float(np.min(y))
    p = dict(X=X, y=y, st=st, C=C, sel=np.arange(1000), mu_x=mu_x.astype(np.float64), sd_x=sd_x.astype(np.float64),
             scale=_mu_scale(st, C), ei=_ei_host(st, C, y_opt), y_opt=y_opt)
    for a in (C, p["ei"]):
        a.setflags(write=False)
    return p


@pytest.mark.parametrize("n,d", [(1, 2), (16, 2), (17, 5), (48, 5), (64, 10), (65, 10), (80, 10), (200, 10),
                                 (208, 14), (100, 30)])
def test_prefetch_edges(n, d, monkeypatch):
    """1, 1, 2, 3, 4, 5, 5, 13, 13 and 7 observation blocks over the four shares: shares
    of zero blocks (nothing loaded, nothing waited for), of one block (the prefetch
    re-reads it), the extra block on share 0, and m = 1000 leaves a ragged last tile."""
    _check_parity(_edge_problem(n, d), _score_both(_edge_problem(n, d), monkeypatch), f"n={n} d={d}")


def _grid():
    # the flagship-width instance launches at occupancy 5: five workgroups per CU
    return 5 * torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _mixed_problem():
    n, d = 80, 10
    m = 3 * 16 * _grid() + 5
    X, y = O.synthetic_problem(n, d, seed=n + d)
    ls = _ls(d)
    st = O.gp_from_theta(X, y, AMP, ls, NOISE)
    C = O.synthetic_candidates(m, d, seed=7).copy()
    ntiles = (m + 15) // 16
    far = np.arange(3, ntiles, 7)
    for t in far:
        C[16 * t:16 * t + 16] = C[16 * t:16 * t + 16] * 12.0 - 5.5
    cc = np.sum((C / ls) ** 2, axis=1)
    assert all(np.max(cc[16 * t:16 * t + 16]) > 2.0 for t in far)          # one such row sends the tile to the direct form
    near = np.ones(m, dtype=bool)
    for t in far:
        near[16 * t:16 * t + 16] = False
    assert np.max(cc[near]) <= 1.0
    # the oracle on every 29th tile (29 and 7 are coprime: far and near tiles, both tile
    # parities, all three rounds of the loop) and the ragged last one
    tiles = np.union1d(np.arange(0, ntiles, 29), [ntiles - 1])
    assert np.intersect1d(tiles, far).size >= 8
    sel = np.concatenate([np.arange(16 * t, min(16 * t + 16, m)) for t in tiles])
    mu_x, sd_x = O.posterior_exact(st, C[sel])
    y_opt = float(np.min(y))
    p = dict(X=X, y=y, st=st, C=C, sel=sel, mu_x=mu_x.astype(np.float64), sd_x=sd_x.astype(np.float64),
             scale=_mu_scale(st, C[sel]), ei=_ei_host(st, C, y_opt), y_opt=y_opt)
    for a in (C, p["ei"]):
        a.setflags(write=False)
    return p


def test_mixed_tiles_in_one_loop(monkeypatch):
    """n = 80 (five blocks: share 0 carries two), three tiles per workgroup and a ragged
    last one; every seventh tile is far (|c / ls|^2 > 2), so one wave alternates between
    the prefetching loop and the direct form across both tile parities."""
    p = _mixed_problem()
    _check_parity(p, _score_both(p, monkeypatch), f"mixed m={p['C'].shape[0]}")


@pytest.mark.parametrize("far_tile", [False, True])
def test_position_independence(far_tile):
    """64 distinct rows repeated over the whole batch: mu, sd and EI of every repeat are
    bit-equal to the first.  A prefetch register consumed early or late shows as a value
    that depends on the tile's place in a workgroup's loop.  (q's fold order follows
    blockIdx.x & 3; a period of 64 rows = 4 tiles keeps that fixed while the grid is a
    multiple of four workgroups.  The parent commit holds this too.)  far_tile: the
    fourth tile of the period is far, so a quarter of the workgroups run the direct form."""
    from mpi_opt_amd.gp import DeviceGP

    n, d = 80, 10
    assert _grid() % 4 == 0
    m = 3 * 16 * _grid() + 5
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, AMP, _ls(d), NOISE)
    block = O.synthetic_candidates(64, d, seed=3).copy()
    if far_tile:
        block[48:] = block[48:] * 12.0 - 5.5
        assert np.max(np.sum((block[48:] / st.length_scale) ** 2, axis=1)) > 2.0
    reps = (m + 63) // 64
    C = torch.tensor(np.tile(block, (reps, 1))[:m], device="cuda")
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    assert g.score_path == 0 and g.model.xb
    out = g.score(C, float(np.min(y)), acqs=("EI",), k=5)
    torch.cuda.synchronize()
    for name, t in (("mu", out["mu"]), ("sd", out["sd"]), ("EI", out["values"]["EI"])):
        first = t[:64]
        full = t[:(m // 64) * 64].reshape(-1, 64)
        bad = int(torch.count_nonzero(full != first))
        tail = int(torch.count_nonzero(t[(m // 64) * 64:] != first[:m % 64]))
        print(f"far_tile={far_tile} {name}: entries differing from the first repeat {bad} + {tail}")
        assert bad == 0 and tail == 0
    # and the first repeat is the posterior
    mu_x, sd_x = O.posterior_exact(st, block)
    assert np.max(np.abs(out["mu"][:64].cpu().numpy() - mu_x.astype(np.float64)) / _mu_scale(st, block)) < 1e-9
    assert np.max(np.abs(out["sd"][:64].cpu().numpy() - sd_x.astype(np.float64)) / sd_x.astype(np.float64)) < 1e-9
