"""GPU parity of the pathwise posterior samples (``mpo_gp_paths_prepare`` / ``mpo_gp_paths_eval``,
``DeviceGP.paths`` / ``DevicePaths.eval``) against the chain of tests/paths_ref.py in 80-bit.

Bars: every sample within 1e-9 y_std sqrt(amp) (the bar tests/test_gp_joint_gpu.py holds
``mpo_gp_sample`` to), every draw's argmin the exact one and ``np.argmin`` of the device's own
rows, ``minval`` the row's minimum bit for bit.  Every case first checks its reference alone:
the fp64 restatement within 1e-10 of the 80-bit chain and a best-to-second gap >= 1e-6.

The kernel's edges (csrc/gp_paths.hip): 64-candidate tiles, 16-draw tiles (a wave's second
tile starts at draw 64), 256 draws per workgroup, features padded to 16, 64-column panels of
[features | observations], and a grid that loops once m / 64 passes its cap (MPO_PATHS_GRID).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import joint_cases as J
from tests import paths_ref as R

pytestmark = pytest.mark.gpu

SEED = 11


@functools.lru_cache(maxsize=None)
def case(n, d, m, s, F, seed=SEED):
    """Inputs and the 80-bit samples of a case, shared between the tests: never written."""
    X, y, C, _ = J.inputs(n, d, m)
    amp, ls, noise = J.theta(d)
    rnd = R.draw_paths(np.random.RandomState(seed), F, d, s, n)
    S_x, arg = R.samples(X, y, C, amp, ls, noise, *rnd, precision="exact")
    S_64, _ = R.samples(X, y, C, amp, ls, noise, *rnd, precision="fp64")
    scale = R.normalise(y)[1] * np.sqrt(amp)
    e_ref = float(np.max(np.abs(S_64 - S_x))) / scale
    gap = R.gap_of(S_x, scale)
    print(f"(n, d, m, s, F) = {(n, d, m, s, F)}: fp64 vs 80-bit {e_ref:.3e}, smallest gap {gap:.3e}, "
          f"max |omega . c + phase| {arg:.3g}")
    assert e_ref <= R.REF_BAR and gap >= R.ARGMIN_GAP
    return {"X": X, "y": y, "C": C, "theta": (amp, ls, noise), "rnd": rnd, "S": S_x, "scale": scale}


def device(c, g=None):
    from mpi_opt_amd.gp import DeviceGP

    amp, ls, noise = c["theta"]
    g = g if g is not None else DeviceGP(c["X"], c["y"], amp, ls, noise)
    return g, g.paths(*c["rnd"], noise=noise)


def check(c, out, S_ref=None, rows=slice(None), draws=slice(None)):
    S_ref = (c["S"] if S_ref is None else S_ref)[draws, rows]
    S, am, mv = (out[k].cpu().numpy() for k in ("samples", "argmin", "minval"))
    assert S.shape == S_ref.shape and am.shape == (S.shape[0],) and am.dtype == np.int64
    e = float(np.max(np.abs(S - S_ref))) / c["scale"]
    print(f"samples err {e:.3e} of y_std sqrt(amp), {len(set(am.tolist()))} distinct argmins of {len(am)}")
    assert e <= R.VALUE_BAR
    assert np.array_equal(am, np.argmin(S_ref, axis=1))
    assert np.array_equal(am, np.argmin(S, axis=1))
    assert np.array_equal(mv, S[np.arange(len(am)), am])
    return S, am, mv


# the issue's four cases, then the edges: n = 1, F = 1, s = 1, m = 1; 15 / 16 / 17 at the
# 16 edges of n, s and F; 63 / 64 / 65 at the 64 edges of m, F, n and of a wave's second
# draw tile; 127 / 128 / 129 rows; 255 / 256 / 257 draws (the second workgroup row);
# F + np16 one panel (16 + 48), just past it (17 + 48 -> 32 + 48) and several.
CASES = [(17, 2, 48, 32, 64), (64, 4, 96, 32, 256), (33, 32, 80, 16, 128), (200, 10, 257, 64, 512),
         (1, 2, 1, 1, 1), (15, 2, 63, 15, 15), (16, 4, 64, 16, 16), (17, 2, 65, 17, 17), (48, 3, 127, 3, 16),
         (48, 3, 70, 3, 17), (63, 3, 128, 63, 63), (64, 4, 129, 65, 64), (65, 10, 66, 255, 65),
         (33, 5, 70, 256, 100), (40, 5, 66, 257, 130)]


@pytest.mark.parametrize("n,d,m,s,F", CASES)
def test_samples_and_argmin_match_exact(n, d, m, s, F):
    c = case(n, d, m, s, F)
    check(c, device(c)[1].eval(c["C"], want_samples=True))


def test_capped_grid_loops_over_the_tiles(monkeypatch):
    """m = 330: six candidate tiles over two workgroups, three trips each; the bits of the
    uncapped launch."""
    c = case(33, 5, 330, 17, 100)
    p = device(c)[1]
    whole = check(c, p.eval(c["C"], want_samples=True))
    monkeypatch.setenv("MPO_PATHS_GRID", "2")
    capped = check(c, p.eval(c["C"], want_samples=True))
    monkeypatch.setenv("MPO_PATHS_GRID", "1")
    one = check(c, p.eval(c["C"], want_samples=True))
    for u, v, w in zip(whole, capped, one):
        assert np.array_equal(u, v) and np.array_equal(u, w)


def test_streamed_size_model_against_fp64():
    """n = 1300 is past the 80-bit chain and on the streamed scoring path: the fp64
    restatement at the same bar."""
    n, d, m, s, F = 1300, 5, 64, 16, 64
    X, y, C, _ = J.inputs(n, d, m)
    amp, ls, noise = J.theta(d)
    rnd = R.draw_paths(np.random.RandomState(SEED), F, d, s, n)
    S_64, _ = R.samples(X, y, C, amp, ls, noise, *rnd, precision="fp64")
    scale = R.normalise(y)[1] * np.sqrt(amp)
    gap = R.gap_of(S_64, scale)
    print(f"smallest gap {gap:.3e}")
    assert gap >= R.ARGMIN_GAP
    c = {"X": X, "y": y, "C": C, "theta": (amp, ls, noise), "rnd": rnd, "S": S_64, "scale": scale}
    g, p = device(c)
    assert g.score_path == 1
    check(c, p.eval(C, want_samples=True))


def test_short_length_scale():
    """ls = 0.02 in one dimension over [0, 10]: |omega . c + phase| passes 1e3, the cosine's
    range reduction is a real one.  Half the observations have a candidate within a length
    scale, so the Matern columns matter too."""
    n, m, s, F = 24, 70, 16, 64
    rs = np.random.RandomState(4)
    X = rs.uniform(0.0, 10.0, (n, 1))
    y = np.sin(9.0 * X[:, 0]) + 0.1 * rs.standard_normal(n)
    C = rs.uniform(0.0, 10.0, (m, 1))
    C[:n // 2, 0] = X[:n // 2, 0] + 0.01 * rs.standard_normal(n // 2)
    amp, ls, noise = 2.0, np.array([0.02]), 0.05
    rnd = R.draw_paths(np.random.RandomState(SEED), F, 1, s, n)
    S_x, arg = R.samples(X, y, C, amp, ls, noise, *rnd, precision="exact")
    S_64, _ = R.samples(X, y, C, amp, ls, noise, *rnd, precision="fp64")
    scale = R.normalise(y)[1] * np.sqrt(amp)
    e_ref, gap = float(np.max(np.abs(S_64 - S_x))) / scale, R.gap_of(S_x, scale)
    print(f"largest |omega . c + phase| {arg:.4g}; fp64 vs 80-bit {e_ref:.3e}, smallest gap {gap:.3e}")
    assert arg > 1e3 and e_ref <= R.REF_BAR and gap >= R.ARGMIN_GAP
    c = {"X": X, "y": y, "C": C, "theta": (amp, ls, noise), "rnd": rnd, "S": S_x, "scale": scale}
    check(c, device(c)[1].eval(C, want_samples=True))


def test_rows_and_draws_alone_give_the_bits_of_the_whole():
    c = case(40, 5, 330, 40, 130)
    g, p = device(c)
    S, am, mv = check(c, p.eval(c["C"], want_samples=True))
    for a, b in ((1, 330), (37, 101), (63, 65), (64, 128), (65, 329), (200, 201)):
        out = p.eval(c["C"][a:b], want_samples=True)
        assert np.array_equal(out["samples"].cpu().numpy(), S[:, a:b]), (a, b)
        assert np.array_equal(out["argmin"].cpu().numpy(), np.argmin(S[:, a:b], axis=1))
    for k, nd in ((0, 1), (5, 1), (39, 1), (3, 17), (16, 17), (23, 17)):
        out = p.eval(c["C"], first_draw=k, n_draws=nd, want_samples=True)
        assert np.array_equal(out["samples"].cpu().numpy(), S[k:k + nd]), (k, nd)
        assert np.array_equal(out["argmin"].cpu().numpy(), am[k:k + nd])
        assert np.array_equal(out["minval"].cpu().numpy(), mv[k:k + nd])
    # without the sample rows: the same fold
    out = p.eval(c["C"])
    assert out["samples"] is None
    assert np.array_equal(out["argmin"].cpu().numpy(), am) and np.array_equal(out["minval"].cpu().numpy(), mv)


def test_two_calls_give_the_same_bits():
    c = case(200, 10, 257, 64, 512)
    g, p = device(c)
    a = p.eval(c["C"], want_samples=True)
    b = device(c)[1].eval(c["C"], want_samples=True)
    e = p.eval(c["C"], want_samples=True)
    for k in ("samples", "argmin", "minval"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], e[k])


def test_appended_model_and_factor_copy():
    """An appended model (chain 24 -> 40, d = 10) meets the bars; a from_factor copy of it
    gives its bits (and needs the noise spelled out)."""
    from mpi_opt_amd.gp import DeviceGP

    c = case(40, 10, 96, 32, 128)
    g = J.device_gp(c["X"][:24], c["y"][:24], 10)
    for k in range(24, 40):
        g = g.appended(c["X"][k], c["y"][:k + 1])
    _, p = device(c, g)
    S, am, mv = check(c, p.eval(c["C"], want_samples=True))
    meta, layout, ws = g.export_factor()
    copy = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=ws.device)[256:]
    copy.copy_(ws)
    h = DeviceGP.from_factor(meta, layout, copy)
    assert h.model.W != g.model.W
    with pytest.raises(ValueError, match="noise"):
        h.paths(*c["rnd"])
    out = h.paths(*c["rnd"], noise=c["theta"][2]).eval(c["C"], want_samples=True)
    assert np.array_equal(out["samples"].cpu().numpy(), S) and np.array_equal(out["argmin"].cpu().numpy(), am)


def test_streamed_model_in_a_fresh_process_gives_the_same_bits(tmp_path):
    """Only W, xs, alpha and ls are read: a model prepared under MPO_GP_SCORE=streamed (read at
    prepare time, so in a fresh child process) gives the bits of the default path."""
    from mpi_opt_amd.gp import DeviceGP

    X, y, C, (amp, ls, noise), rnd = R.path_case()
    g = DeviceGP(X, y, amp, ls, noise)
    assert g.score_path == 0
    here = g.paths(*rnd).eval(C, want_samples=True)
    out = str(tmp_path / "streamed.npz")
    env = dict(os.environ, MPO_GP_SCORE="streamed")
    subprocess.run([sys.executable, os.path.join(R.ROOT, "tests", "paths_ref.py"), out], env=env, check=True,
                   timeout=240)
    there = np.load(out)
    assert int(there["score_path"]) == 1
    for name in ("samples", "argmin", "minval"):
        assert np.array_equal(there[name], here[name].cpu().numpy()), name


def test_ties_go_to_the_lowest_index():
    """Duplicated candidate rows have equal samples, bit for bit: the argmin is the first."""
    c = case(17, 2, 65, 17, 17)
    p = device(c)[1]
    base = c["C"]
    am0 = p.eval(base)["argmin"].cpu().numpy()
    # every row three times, copies first in another tile and last in the same one
    C = np.vstack([base, base[::-1], base])
    out = p.eval(C, want_samples=True)
    S, am = out["samples"].cpu().numpy(), out["argmin"].cpu().numpy()
    assert np.array_equal(S[:, :65], S[:, 130:]) and np.array_equal(S[:, :65], S[:, 129:64:-1])
    assert np.array_equal(am, am0) and np.array_equal(am, np.argmin(S, axis=1))
    C2 = np.repeat(base[am0[:1]], 200, axis=0)              # one row 200 times: index 0
    out = p.eval(C2)
    assert np.array_equal(out["argmin"].cpu().numpy(), np.zeros(17, dtype=np.int64))


def test_sample_paths_is_a_function():
    """GPModel.sample_paths: (m, n_samples), the same values wherever a point is evaluated."""
    from mpi_opt_amd.optimizer import GPModel

    c = case(17, 2, 48, 32, 64)
    amp, ls, noise = c["theta"]
    est = GPModel(c["X"], c["y"], amp, ls, noise)
    f = est.sample_paths(n_samples=3, n_features=64, random_state=SEED)
    A = f(c["C"])
    assert A.shape == (48, 3)
    assert np.array_equal(f(c["C"][5:9]), A[5:9]) and np.array_equal(f(c["C"][7]), A[7:8])
    rnd = R.draw_paths(np.random.RandomState(SEED), 64, 2, 3, 17)
    S_x, _ = R.samples(c["X"], c["y"], c["C"], amp, ls, noise, *rnd, precision="exact")
    assert float(np.max(np.abs(A.T - S_x))) <= R.VALUE_BAR * c["scale"]
