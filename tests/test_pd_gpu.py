"""``mpo_gp_partial_dependence`` on the device against the restatements of tests/pd_ref.py
(fixtures: tests/pd_cases.py; stored 80-bit values: tests/golden/pd_ref.npz).

Bars, all as multiples of a cell's summand scale ``y_std (1 / S) sum_s sum_i |alpha_i| amp k_si``:

* the kernel alone, against the 80-bit definition on the DEVICE model's own alpha, xs and ls
  (the factor's error stays out): ``max(1e-12, 16 x the fp64 restatement's own error)``.  A
  fixed-order two-level sum of n <= 2048 by S <= 250 terms is bounded by (n + S) 2^-52 ~ 5e-13
  of the scale, plus a few ulp per Matern value;
* against ``DeviceGP.predict``'s mean at the materialised rows: 1e-9, the project's posterior bar;
* end to end against the exact factor's alpha: ``max(1e-9, 4 x the fp64 restatement's error)``.
"""
import ctypes

import numpy as np
import pytest

from tests import pd_cases as C
from tests import pd_ref as R

pytestmark = pytest.mark.gpu

MPO_EINVAL = 1


@pytest.fixture(scope="module")
def gpu():
    import torch

    from mpi_opt_amd import _lib, gp
    return torch, _lib, gp


_GPS = {}


def device_gp(n, d, far=False):
    from mpi_opt_amd.gp import DeviceGP

    if (n, d, far) not in _GPS:
        X, y, (amp, ls, noise) = C.inputs(n, d, far)
        _GPS[(n, d, far)] = DeviceGP(np.array(X), y, amp, ls, noise, device="cuda:0")
    return _GPS[(n, d, far)]


def samples(*case):
    """A writable copy of the fixture's rows (the fixtures are read-only; torch wants writable arrays)."""
    return np.array(C.samples(*case))


def model_arrays(g):
    """The device model's own (xs [n][d], ls [d], alpha [n]) as numpy."""
    dp = g.model.dp
    xs = g._state_view(g.model.xs, g.n * dp).view(g.n, dp).cpu().numpy()[:, :g.d]
    ls = g._state_view(g.model.ls, g.d).cpu().numpy()
    return xs, ls, g.alpha().cpu().numpy()


# ---- 1. the kernel alone -----------------------------------------------------------------------
@pytest.mark.parametrize("n,d,S", C.KERNEL_CASES, ids=lambda v: str(v))
def test_kernel_parity(n, d, S, gpu):
    far = (n, d, S) == C.FAR_CASE
    g = device_gp(n, d, far)
    xs, ls, alpha = model_arrays(g)
    assert np.array_equal(ls, C.inputs(n, d, far)[2][1])
    if far:
        assert np.max(np.sum(xs * xs, axis=1)) > 100.0            # |x / ls|^2 >> 2
    smp, tasks = samples(n, d, S, far), C.kernel_tasks(n, d, S)
    got = g.partial_dependence(smp, tasks)
    assert len(got) == len(tasks)
    for j, (task, v) in enumerate(zip(tasks, got)):
        assert v.shape == R.shape_of(task) and np.all(np.isfinite(v))
        ref, scale = R.pd_exact(xs, ls, alpha, g.amp, g.y_mean, g.y_std, smp, task, scaled=True)
        v64 = R.pd_fp64(xs, ls, alpha, g.amp, g.y_mean, g.y_std, smp, task, scaled=True)
        assert np.all(scale > 0)
        err64 = R.rel_err(v64, ref, scale)
        bar = np.maximum(1e-12, 16 * err64)
        err = R.rel_err(v, ref, scale)
        print(f"PD-KERNEL ({n}, {d}, {S}) task {j} {v.shape}: worst error {np.max(err):.3e} of the scale, "
              f"{np.max(err / bar):.3e} of its bar; fp64 restatement {np.max(err64):.3e}")
        assert np.all(err <= bar), (n, d, S, j, float(np.max(err / bar)))


# ---- 2. the same posterior as predict ------------------------------------------------------------
def test_flagship_tasks_against_predict(gpu):
    n, d, S = 200, 10, 250
    g = device_gp(n, d)
    xs, ls, alpha = model_arrays(g)
    smp = samples(n, d, S)
    tasks = [(2, C.lin(6), 8, C.lin(5)), (4, C.lin(40))]
    got = g.partial_dependence(smp, tasks)
    for j, (task, v) in enumerate(zip(tasks, got)):
        cells = R.cells_of(task)
        rows = np.vstack([R.rows_of(smp, task, c) for c in cells])
        mu = g.predict(rows, return_std=False).reshape(len(cells), S).mean(axis=1).reshape(v.shape)
        scale = R.pd_exact(xs, ls, alpha, g.amp, g.y_mean, g.y_std, smp, task, scaled=True)[1]
        err = np.abs(v - mu) / scale
        print(f"PD-PREDICT task {j}: worst |fused - mean of predict| {np.max(err):.3e} of the scale (bar 1e-9)")
        assert np.all(err <= 1e-9)


@pytest.mark.parametrize("n,d,S", C.GOLDEN_CASES, ids=lambda v: str(v))
def test_end_to_end_against_the_exact_factor(n, d, S, gpu):
    gold = C.golden()
    g = device_gp(n, d)
    tasks = C.golden_tasks(n, d)
    got = g.partial_dependence(samples(n, d, S), tasks)
    for j, v in enumerate(got):
        k = C.key(n, d, S, j)
        ref = C.join(gold[k + "_hi"], gold[k + "_lo"])
        bar = np.maximum(1e-9, 4 * gold[k + "_err64"])
        err = R.rel_err(v, ref, gold[k + "_scale"])
        print(f"PD-E2E {k}: worst error {np.max(err):.3e} of the scale, {np.max(err / bar):.3e} of its bar")
        assert np.all(err <= bar), (k, float(np.max(err / bar)))


# ---- 3. isolation and determinism ----------------------------------------------------------------
def _raw(gpu, g, smp, table, T, grid, total, ws_bytes=None, sentinel=-7.25, guard=4096):
    """One ctypes call into a sentinel-filled output and a guarded workspace:
    (rc, out numpy, the guard bytes after the workspace)."""
    torch, _lib, gp = gpu
    L = _lib.lib()
    s = g.as_candidates(smp)
    need = L.mpo_gp_pd_ws_bytes(ctypes.byref(g.model), s.shape[0], table, T)
    assert need > 0
    use = need if ws_bytes is None else ws_bytes
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
    gd = torch.from_numpy(np.ascontiguousarray(grid)).cuda()
    out = torch.full((total,), sentinel, dtype=torch.float64, device="cuda:0")
    rc = L.mpo_gp_partial_dependence(ctypes.byref(g.model), s.data_ptr(), s.shape[0], table, T, gd.data_ptr(),
                                     out.data_ptr(), ws.data_ptr(), use, _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), ws[need:].cpu().numpy()


def test_a_task_keeps_its_bits_wherever_it_stands(gpu):
    torch, _lib, gp = gpu
    n, d, S = 200, 10, 250
    g = device_gp(n, d)
    smp = samples(n, d, S)
    # the 55-task list at a reduced grid (the positions are what is tested); the probe tasks at 0, 27, 54
    base = C.flagship_tasks(d, 6)
    probe_1d, probe_2d = (7, C.lin(40)), (1, C.lin(40), 6, C.lin(13))
    alone = [g.partial_dependence(smp, [t])[0] for t in (probe_1d, probe_2d)]
    for probe, want in zip((probe_1d, probe_2d), alone):
        for pos in (0, 27, 54):
            tasks = list(base)
            tasks[pos] = probe
            assert len(tasks) == 55
            got = g.partial_dependence(smp, tasks)
            assert got[pos].tobytes() == want.tobytes(), (len(probe), pos)
    # two calls, and another model's call in between
    tasks = list(base)
    first = g.partial_dependence(smp, tasks)
    other = device_gp(17, 3)
    other.partial_dependence(samples(17, 3, 7), C.golden_tasks(17, 3))
    second = g.partial_dependence(smp, tasks)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_output_outside_the_tasks_keeps_its_sentinel(gpu):
    torch, _lib, gp = gpu
    n, d, S = 17, 3, 7
    g = device_gp(n, d)
    table, grid, shapes, total = gp.pd_table(C.golden_tasks(n, d))
    # spread the outputs: a hole of 3 doubles in front of every task and 5 behind the last
    off = 0
    for t, shp in enumerate(shapes):
        off += 3
        table[t].out_off = off
        off += int(np.prod(shp))
    rc, out, _ = _raw(gpu, g, samples(n, d, S), table, len(shapes), grid, off + 5)
    assert rc == 0
    want = g.partial_dependence(samples(n, d, S), C.golden_tasks(n, d))
    covered = np.zeros(off + 5, dtype=bool)
    for t, shp in enumerate(shapes):
        k = int(np.prod(shp))
        assert out[table[t].out_off:table[t].out_off + k].tobytes() == want[t].tobytes()
        covered[table[t].out_off:table[t].out_off + k] = True
    assert np.all(out[~covered] == -7.25) and (~covered).sum() == 3 * len(shapes) + 5


# ---- 4. workspace --------------------------------------------------------------------------------
def test_workspace_is_exact_and_guarded(gpu):
    torch, _lib, gp = gpu
    n, d, S = 200, 10, 250
    g = device_gp(n, d)
    tasks = C.golden_tasks(n, d) + [(0, C.lin(64), 9, C.lin(40))]
    table, grid, shapes, total = gp.pd_table(tasks)
    need = _lib.lib().mpo_gp_pd_ws_bytes(ctypes.byref(g.model), S, table, len(shapes))
    rc, out, guard = _raw(gpu, g, samples(n, d, S), table, len(shapes), grid, total)
    assert rc == 0 and np.all(guard == 0x5A) and np.all(out != -7.25)
    rc, out, guard = _raw(gpu, g, samples(n, d, S), table, len(shapes), grid, total, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in _lib.lib().mpo_last_error()
    assert np.all(out == -7.25) and np.all(guard == 0x5A)
