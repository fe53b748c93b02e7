"""The resident scoring kernel under static wave priorities.

The kernel raises its waves' priority outside phase 2 and lowers it for the MFMA
stream.  No value depends on that, but the order in which the waves of the resident
workgroups make progress does, and the tile loop leans on that order in places that
carry no barrier of their own: the mu rows alternate between two halves of ``red`` by
tile parity, the q rows are rewritten behind barrier B, the next tile's candidate rows
go into ``cs`` between the barriers, phase 1's operand loads and phase 2's ring are
asm loads tied to explicit waits.  A reuse that only held because the waves happened
to run in step shows up as a value that depends on where a row sits in the batch.

Bars: those of tests/test_gp_score_tile_path_gpu.py -- mu (relative to its summand
scale) and sd within 1e-9 of the oracle's extended-precision posterior, the MFMA
distance against the direct form within 1e-10, the top-5 identical between the two
forms, bit-equal repeats where a case repeats rows.

Cases:
  column tiles     n = 1, 16, 17, 33, 200, 208, 209 (one column tile with three empty
                   streams; tiles of one group; T = 13; a multiple of 16; T = 14 with an
                   uneven wave plan), d = 10 (MFMA distance) and 14 (direct), m = 1000;
                   n = 33 again with three tiles per workgroup and a ragged last one
  Matern clamp     n = 80, d = 10: in tile r (r = 0..3) rows 4r..4r+3 are exact copies of
                   observation rows, so the clamped r^2 = 0 sits in exactly one of the four
                   accumulator registers of the distance tile
  tile-loop rounds n = 16, d = 5, 10, 30 (two, three and four waves load candidate rows,
                   one or two elements per thread), m = k 16 grid + r for k = 1..4 and
                   r = -1, 0, +1: prologue only, one to three loop rounds, a ragged or
                   missing last tile; 64 distinct rows repeated over the batch
  far tiles        n = 16, 17, 48, 64, 65, 80 (shares of zero, one and two blocks), three
                   tiles per workgroup, every seventh tile far (|c / ls|^2 > 2) so a wave
                   alternates between the MFMA-distance loop and the direct form; one case
                   with the last tile far"""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_ei as O
from tests import test_gp_score_tile_path_gpu as T
from tests.test_gp_score_shapes_gpu import xb_flag

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [10, 14])
@pytest.mark.parametrize("n", [1, 16, 17, 33, 200, 208, 209])
def test_column_tile_boundaries(n, d, monkeypatch):
    p = T._edge_problem(n, d)
    T._check_parity(p, T._score_both(p, monkeypatch), f"n={n} d={d}")


@functools.lru_cache(maxsize=None)
def _loop_problem(n, far_every, last_far):
    """Three tiles per workgroup and a ragged last one; optionally every ``far_every``-th
    tile (from tile 3) and / or the last tile far.  The oracle runs on every 59th tile, the
    first eight far ones and the last."""
    d = 10
    m = 3 * 16 * T._grid() + 5
    X, y = O.synthetic_problem(n, d, seed=n + d)
    ls = T._ls(d)
    st = O.gp_from_theta(X, y, T.AMP, ls, T.NOISE)
    C = O.synthetic_candidates(m, d, seed=7).copy()
    ntiles = (m + 15) // 16
    far = list(range(3, ntiles - 1, far_every)) if far_every else []
    if last_far:
        far.append(ntiles - 1)
    near = np.ones(m, dtype=bool)
    for t in far:
        C[16 * t:16 * t + 16] = C[16 * t:16 * t + 16] * 12.0 - 5.5
        near[16 * t:16 * t + 16] = False
    cc = np.sum((C / ls) ** 2, axis=1)
    assert all(np.max(cc[16 * t:16 * t + 16]) > 2.0 for t in far)
    assert np.max(cc[near]) <= 1.0
    tiles = np.union1d(np.union1d(np.arange(0, ntiles, 59), far[:8] + far[-1:]), [ntiles - 1]).astype(int)
    sel = np.concatenate([np.arange(16 * t, min(16 * t + 16, m)) for t in tiles])
    mu_x, sd_x = O.posterior_exact(st, C[sel])
    y_opt = float(np.min(y))
    p = dict(X=X, y=y, st=st, C=C, sel=sel, mu_x=mu_x.astype(np.float64), sd_x=sd_x.astype(np.float64),
             scale=T._mu_scale(st, C[sel]), ei=T._ei_host(st, C, y_opt), y_opt=y_opt)
    for a in (C, p["ei"]):
        a.setflags(write=False)
    return p


def test_column_tiles_of_one_group_over_three_rounds(monkeypatch):
    p = _loop_problem(33, None, False)
    T._check_parity(p, T._score_both(p, monkeypatch), "n=33 three rounds")


@pytest.mark.parametrize("n", [16, 17, 48, 64, 65, 80])
def test_far_tiles_between_near_ones(n, monkeypatch):
    p = _loop_problem(n, 7, False)
    T._check_parity(p, T._score_both(p, monkeypatch), f"n={n} every seventh tile far")


def test_last_tile_far(monkeypatch):
    p = _loop_problem(80, 7, True)
    T._check_parity(p, T._score_both(p, monkeypatch), "n=80 last tile far")


def test_clamped_distance_in_one_accumulator_register(monkeypatch):
    n, d = 80, 10
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, T.AMP, T._ls(d), T.NOISE)
    C = O.synthetic_candidates(1000, d, seed=11).copy()
    for r in range(4):
        C[16 * r + 4 * r:16 * r + 4 * r + 4] = X[5 * r:5 * r + 4]      # tile r: rows 4r .. 4r + 3
    mu_x, sd_x = O.posterior_exact(st, C)
    y_opt = float(np.min(y))
    p = dict(X=X, y=y, st=st, C=C, sel=np.arange(1000), mu_x=mu_x.astype(np.float64), sd_x=sd_x.astype(np.float64),
             scale=T._mu_scale(st, C), ei=T._ei_host(st, C, y_opt), y_opt=y_opt)
    out = T._score_both(p, monkeypatch)
    assert xb_flag(out["1"][0]) == 1.0           # the model's self-check of the expanded distance
    T._check_parity(p, out, "clamped r2 per register")


@pytest.mark.parametrize("d", [5, 10, 30])
def test_tile_loop_rounds(d):
    from mpi_opt_amd.gp import DeviceGP

    n, grid = 16, T._grid()
    assert grid % 4 == 0                         # q's fold order follows blockIdx.x & 3: 64 rows = 4 tiles keep it fixed
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, T.AMP, T._ls(d), T.NOISE)
    block = O.synthetic_candidates(64, d, seed=3)
    mu_x, sd_x = O.posterior_exact(st, block)
    mu_x, sd_x = mu_x.astype(np.float64), sd_x.astype(np.float64)
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    assert g.score_path == 0 and bool(g.model.xb) == (d + 2 <= g.model.dp)
    for k in (1, 2, 3, 4):
        for r in (-1, 0, 1):
            m = k * 16 * grid + r
            C = torch.tensor(np.tile(block, ((m + 63) // 64, 1))[:m], device="cuda")
            out = g.score(C, float(np.min(y)), acqs=("EI",), k=5)
            torch.cuda.synchronize()
            bad = 0
            for t in (out["mu"], out["sd"], out["values"]["EI"]):
                first = t[:64]
                bad += int(torch.count_nonzero(t[:(m // 64) * 64].reshape(-1, 64) != first))
                bad += int(torch.count_nonzero(t[(m // 64) * 64:] != first[:m % 64]))
            e_mu = np.max(np.abs(out["mu"][:64].cpu().numpy() - mu_x) / T._mu_scale(st, block))
            e_sd = np.max(np.abs(out["sd"][:64].cpu().numpy() - sd_x) / sd_x)
            print(f"d={d} m={m}: entries differing from the first repeat {bad}  mu err {e_mu:.3e}  sd err {e_sd:.3e}")
            assert bad == 0
            assert e_mu < 1e-9 and e_sd < 1e-9
