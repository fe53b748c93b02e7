"""Host side of the objective report (no GPU): the fp64 restatement of the partial-dependence
kernel's decomposition against the stored 80-bit definition, ``mpo_gp_partial_dependence``'s
refusals on host structs, the grid rule per dimension kind, the orientation of ``zi``, the
``--report`` flag and ``plot_report``.

The restatement's bar: 1e-15 of a cell's summand scale (tests/pd_ref.py); measured when the
fixtures were made: 1.0e-16 .. 1.2e-16 at (17, 3, 7), 1.2e-16 at (200, 10, 250), 4.7e-17 at
(600, 6, 64)."""
import ctypes

import numpy as np
import pytest

from mpi_opt_amd import _lib, analysis
from mpi_opt_amd.gp import pd_table
from mpi_opt_amd.search import make_parser
from mpi_opt_amd.space import Categorical, Integer, Real, Space
from tests import pd_cases as C
from tests import pd_ref as R

MPO_EINVAL, MPO_ENOTSUP = 1, 3


# ---- the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,S", C.GOLDEN_CASES, ids=lambda v: str(v))
def test_fp64_restatement_against_the_80_bit_definition(n, d, S):
    g = C.golden()
    X, y, (amp, ls, noise) = C.inputs(n, d)
    alpha = C.join(g[f"alpha_{n}_{d}_hi"], g[f"alpha_{n}_{d}_lo"]).astype(np.float64)
    for j, task in enumerate(C.golden_tasks(n, d)):
        k = C.key(n, d, S, j)
        v = R.pd_fp64(X, ls, alpha, amp, float(np.mean(y)), float(np.std(y)), C.samples(n, d, S), task)
        err = R.rel_err(v, C.join(g[k + "_r_hi"], g[k + "_r_lo"]), g[k + "_scale"])
        print(f"PD-RESTATEMENT {k}: worst error {np.max(err):.3e} of the summand scale (bar 1e-15)")
        assert v.shape == R.shape_of(task) and np.all(err <= 1e-15), (k, float(np.max(err)))
        assert np.array_equal(err, g[k + "_err64"])                     # what the GPU bars are built on


def test_the_two_restatements_agree_on_a_scaled_model():
    """``scaled=True`` (a device model's own xs) is the same arithmetic as raw X / ls."""
    n, d, S = 17, 3, 7
    X, y, (amp, ls, noise) = C.inputs(n, d)
    alpha = np.random.RandomState(0).randn(n)
    task = C.golden_tasks(n, d)[1]
    a = R.pd_fp64(X, ls, alpha, amp, 0.5, 2.0, C.samples(n, d, S), task)
    b = R.pd_fp64(X / ls, ls, alpha, amp, 0.5, 2.0, C.samples(n, d, S), task, scaled=True)
    assert a.tobytes() == b.tobytes()
    e, scale = R.pd_exact(X / ls, ls, alpha, amp, 0.5, 2.0, C.samples(n, d, S), task, scaled=True)
    assert np.all(R.rel_err(a, e, scale) <= 1e-15)


# ---- the ABI's refusals ----------------------------------------------------------------------------
def base(n=10, d=10, dp=12, prepared=True):
    m = _lib.MpoGpModel(n=n, d=d, dp=dp, np16=(n + 15) // 16 * 16, amp=1.0, y_std=1.0)
    if prepared:
        m.xs = m.ls = m.alpha = 64          # never followed: every call below is refused on the host
    return m


@pytest.fixture
def buf():
    b = ctypes.create_string_buffer(64)
    yield ctypes.addressof(b)
    del b


def call(model, S, table, T, p, ws_bytes=1 << 40, samples=True, grid=True, out=True, ws=True):
    """(status, message, ws_bytes query) of one call on host structs; no launch is reached."""
    L = _lib.lib()
    mref = ctypes.byref(model) if model is not None else None
    rc = L.mpo_gp_partial_dependence(mref, p if samples else None, S, table, T, p if grid else None,
                                     p if out else None, p if ws else None, ws_bytes, None)
    return rc, L.mpo_last_error(), L.mpo_gp_pd_ws_bytes(mref, S, table, T)


def one(**kw):
    """A valid one-task table over d = 10, with fields of the task overridden."""
    table, _, _, _ = pd_table([(2, np.linspace(0, 1, 5), 7, np.linspace(0, 1, 4))])
    for name, v in kw.items():
        obj, field = (table[0], name) if "." not in name else (getattr(table[0], name.split(".")[0]), name.split(".")[1])
        setattr(obj, field, v)
    return table


def test_a_valid_query_is_answered_and_only_the_workspace_is_short(buf):
    rc, msg, need = call(base(), 250, one(), 1, buf, ws_bytes=64)
    assert need > 64 and need % 256 == 0
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    rc, msg, _ = call(base(), 250, one(), 1, buf, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    # the scaled samples and one partial per cell and split: 250 x 10 + 4 x 20 doubles
    assert need == (250 * 10 * 8 + 255) // 256 * 256 + (4 * 20 * 8 + 255) // 256 * 256


def test_null_and_unprepared(buf):
    assert call(None, 250, one(), 1, buf)[::2] == (MPO_EINVAL, 0)
    assert call(base(), 250, None, 1, buf)[::2] == (MPO_EINVAL, 0)
    rc, msg, need = call(base(prepared=False), 250, one(), 1, buf)
    assert (rc, need) == (MPO_EINVAL, 0) and b"not prepared" in msg
    assert call(base(0), 250, one(), 1, buf)[::2] == (MPO_EINVAL, 0)
    assert call(base(10, d=10, dp=10), 250, one(), 1, buf)[::2] == (MPO_EINVAL, 0)       # dp is never 10
    for missing in ("samples", "grid", "out", "ws"):
        rc, msg, need = call(base(), 250, one(), 1, buf, **{missing: False})
        assert rc == MPO_EINVAL and b"null" in msg and need > 0, missing


def test_n_past_2048_is_not_supported(buf):
    rc, msg, need = call(base(2049), 250, one(), 1, buf)
    assert (rc, need) == (MPO_ENOTSUP, 0) and b"2048" in msg
    rc, msg, need = call(base(2048), 250, one(), 1, buf, ws_bytes=64)
    assert rc == MPO_EINVAL and b"workspace too small" in msg and need > 0


@pytest.mark.parametrize("S,T", [(0, 1), (-1, 1), (_lib.MPO_PD_SMAX + 1, 1), (250, 0), (250, -3),
                                 (250, _lib.MPO_PD_TMAX + 1)])
def test_s_and_t_ranges(S, T, buf):
    table = (_lib.MpoPdTask * (_lib.MPO_PD_TMAX + 1))()
    for t in range(len(table)):
        table[t].a.col, table[t].a.width, table[t].a.count, table[t].out_off = 0, 1, 1, t
    assert call(base(), S, table, T, buf)[::2] == (MPO_EINVAL, 0)


def test_the_caps_themselves_are_served(buf):
    table = (_lib.MpoPdTask * _lib.MPO_PD_TMAX)()
    for t in range(len(table)):
        table[t].a.col, table[t].a.width, table[t].a.count, table[t].out_off = 0, 1, 1, t
    rc, msg, need = call(base(), _lib.MPO_PD_SMAX, table, _lib.MPO_PD_TMAX, buf, ws_bytes=64)
    assert rc == MPO_EINVAL and b"workspace too small" in msg and need > 0
    assert call(base(), 250, one(**{"a.count": _lib.MPO_PD_GMAX}), 1, buf, ws_bytes=64)[2] > 0


@pytest.mark.parametrize("fields", [
    {"a.width": 0},                                   # an absent first axis
    {"a.col": -1}, {"a.col": 10}, {"a.col": 8, "a.width": 3}, {"b.col": 9, "b.width": 2}, {"b.col": -2},
    {"a.col": 2, "a.width": 6},                       # [2, 8) overlaps b = [7, 8)
    {"a.col": 7}, {"b.col": 2},                       # the same column twice
    {"a.count": 0}, {"a.count": _lib.MPO_PD_GMAX + 1}, {"b.count": 0}, {"b.count": 65}, {"a.count": -1},
    {"a.width": -1}, {"b.width": -1},
    {"a.grid_off": -1}, {"b.grid_off": -8}, {"out_off": -1},
], ids=str)
def test_task_refusals(fields, buf):
    rc, msg, need = call(base(), 250, one(**fields), 1, buf)
    assert (rc, need) == (MPO_EINVAL, 0), (fields, msg)
    assert b"task 0" in msg


def test_overlapping_outputs_are_refused(buf):
    table, _, shapes, _ = pd_table([(0, np.linspace(0, 1, 5)), (1, np.linspace(0, 1, 4), 2, np.linspace(0, 1, 3)),
                                    (3, np.linspace(0, 1, 2))])
    assert call(base(), 250, table, 3, buf, ws_bytes=64)[2] > 0
    table[2].out_off = 16                       # the last cell of task 1 ([5, 17))
    rc, msg, need = call(base(), 250, table, 3, buf)
    assert (rc, need) == (MPO_EINVAL, 0) and b"overlap" in msg
    table[2].out_off, table[0].out_off = 0, 1   # tasks out of order in memory, [0, 2) against [1, 6)
    assert call(base(), 250, table, 3, buf)[::2] == (MPO_EINVAL, 0)
    table[0].out_off = 100                      # disjoint again, in any order
    assert call(base(), 250, table, 3, buf, ws_bytes=64)[2] > 0


# ---- the grid rule ---------------------------------------------------------------------------------
def test_grid_rule_per_dimension_kind():
    xi, g = analysis.dimension_grid(Categorical(["a", "b"]), 40)
    assert list(xi) == [0, 1] and g.shape == (2, 1) and list(g[:, 0]) == [0.0, 1.0]
    xi, g = analysis.dimension_grid(Categorical(["a", "b", "c"]), 40)
    assert list(xi) == [0, 1, 2] and g.shape == (3, 3) and np.array_equal(g, np.eye(3))
    xi, g = analysis.dimension_grid(Categorical(list("abcdefghij")), 4)
    assert list(xi) == [0, 3, 6, 9] and g.shape == (4, 10) and np.array_equal(np.argmax(g, axis=1), xi)
    xi, g = analysis.dimension_grid(Integer(2, 10), 40)
    assert list(xi) == list(range(2, 11)) and g.shape == (9, 1) and np.allclose(g[:, 0], np.arange(9) / 8.0)
    xi, g = analysis.dimension_grid(Integer(0, 100), 5)
    assert list(xi) == [0, 25, 50, 75, 100]
    xi, g = analysis.dimension_grid(Real(-2.0, 6.0), 40)
    assert np.allclose(xi, np.linspace(-2.0, 6.0, 40), rtol=0, atol=1e-14) and np.array_equal(g[:, 0], np.linspace(0, 1, 40))
    xi, g = analysis.dimension_grid(Real(1e-5, 1e-1, prior="log-uniform"), 9)
    assert np.allclose(np.diff(np.log10(xi)), 0.5, rtol=0, atol=1e-12)          # even in the log
    assert np.array_equal(g[:, 0], np.linspace(0, 1, 9)) and xi[0] == 1e-5 and xi[-1] == 1e-1


# ---- zi's orientation ------------------------------------------------------------------------------
class RestatedGP:
    """A DeviceGP stand-in over the fp64 restatement: what analysis.py needs of one."""

    def __init__(self, X, alpha, ls):
        self.X, self.alpha, self.ls, self.n, self.amp = X, alpha, ls, len(X), 1.0
        self.calls = []

    def partial_dependence(self, samples, tasks):
        self.calls.append((np.array(samples), list(tasks)))
        return [R.pd_fp64(self.X, self.ls, self.alpha, 1.0, 0.25, 3.0, samples, t) for t in tasks]

    def mean(self, row):
        K = R.kernel_exact(np.asarray(row, dtype=float).reshape(1, -1), self.X, self.ls, 1.0).astype(np.float64)
        return float(0.25 + 3.0 * (K @ self.alpha)[0])


def test_zi_is_indexed_j_then_i():
    """A model that is steep along dimension 0 and nearly flat along dimension 1, on a space whose
    two grids differ in length: ``zi[jj][ii]`` is the value at (xi[ii], yi[jj])."""
    space = Space([Real(0.0, 2.0, name="steep"), Integer(0, 3, name="flat")])
    X = np.array([[0.1, 0.2], [0.9, 0.7]])
    gp = RestatedGP(X, np.array([1.0, -0.5]), np.array([0.2, 5.0]))
    xi, yi, zi = analysis.partial_dependence(space, gp, 0, 1, n_points=5, x_eval=[1.0, 2])
    assert len(xi) == 5 and list(yi) == [0, 1, 2, 3] and zi.shape == (4, 5)
    for jj, b in enumerate(yi):
        for ii, a in enumerate(xi):
            want = gp.mean(space.transform([[a, b]])[0])
            assert abs(zi[jj, ii] - want) <= 1e-13, (ii, jj)
    assert np.ptp(zi, axis=1).min() > 10 * np.ptp(zi, axis=0).max()          # steep along xi, flat along yi
    # swapped: the transpose, and the 1-D curves of a point are its rows
    yi2, xi2, zi2 = analysis.partial_dependence(space, gp, 1, 0, n_points=5, x_eval=[1.0, 2])
    assert zi2.shape == (5, 4) and np.allclose(zi2, zi.T, rtol=0, atol=1e-15)
    x1, y1 = analysis.partial_dependence(space, gp, 0, n_points=5, x_eval=[1.0, 2])
    assert np.allclose(y1, zi[2], rtol=0, atol=1e-15) and np.array_equal(x1, xi)
    # the samples: x_eval is one row; sample_points are transformed; a seed draws rvs_transformed
    assert gp.calls[0][0].shape == (1, 2) and np.array_equal(gp.calls[0][0], space.transform([[1.0, 2]]))
    analysis.partial_dependence(space, gp, 0, sample_points=[[0.5, 1], [1.5, 3]], n_points=3)
    assert np.array_equal(gp.calls[-1][0], space.transform([[0.5, 1], [1.5, 3]]))
    analysis.partial_dependence(space, gp, 1, n_samples=11, n_points=3, random_state=4)
    assert np.array_equal(gp.calls[-1][0], space.rvs_transformed(11, random_state=np.random.RandomState(4)))
    assert gp.calls[-1][1][0][0] == 1                                           # dimension 1 starts at column 1


def test_categorical_columns_and_spans():
    space = Space([Categorical(["a", "b", "c"]), Real(0.0, 1.0), Categorical(["u", "v"])])
    X = np.random.RandomState(3).uniform(size=(4, 5))
    gp = RestatedGP(X, np.array([0.3, -0.2, 0.5, 0.1]), np.full(5, 0.7))
    xi, yi, zi = analysis.partial_dependence(space, gp, 0, 2, n_samples=6, random_state=1)
    col_a, grid_a, col_b, grid_b = gp.calls[-1][1][0]
    assert (col_a, grid_a.shape, col_b, grid_b.shape) == (0, (3, 3), 4, (2, 1))
    assert list(xi) == [0, 1, 2] and list(yi) == [0, 1] and zi.shape == (2, 3)
    with pytest.raises(ValueError):
        analysis.partial_dependence(space, gp, 1, 1)


# ---- the report without a model, the CLI flag, the plot ------------------------------------------
def test_report_without_a_model():
    from mpi_opt_amd.optimizer import Optimizer

    opt = Optimizer([(0.0, 1.0), (0.0, 1.0)], random_state=0, n_initial_points=4)
    rep = analysis.objective_report(opt)
    assert rep == {"best_observed": None, "seed": 0, "model": None}
    state = opt.rng.get_state()[1].copy()
    opt.tell([0.2, 0.3], 1.5)
    opt.tell([0.4, 0.1], 0.5)
    rep = analysis.objective_report(opt)
    assert rep["best_observed"] == {"x": [0.4, 0.1], "fun": 0.5} and rep["model"] is None
    assert np.array_equal(opt.rng.get_state()[1], state)                      # no draw from the optimizer's stream
    with pytest.raises(ValueError):
        analysis.expected_minimum(opt)


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).report is None
    assert p.parse_args(["--report", "out.json"]).report == "out.json"
    flag = next(a for a in p._actions if "--report" in a.option_strings)
    assert "addition of this build" in flag.help and "NOT in the reference" in flag.help


def test_plot_report_writes_a_png(tmp_path):
    g = [0.0, 0.5, 1.0]
    rep = {"best_observed": {"x": [0.5, 1e-3, "b"], "fun": 0.1}, "expected_minimum": {"x": [0.4, 1e-2, "c"], "fun": 0.05},
           "dimensions": [
               {"name": "lr", "kind": "real", "grid": g, "pd": [0.3, 0.1, 0.4], "importance": 0.3},
               {"name": "wd", "kind": "real", "grid": [1e-4, 1e-3, 1e-2], "pd": [0.2, 0.25, 0.3], "importance": 0.1},
               {"name": None, "kind": "categorical", "grid": [0, 1, 2], "categories": ["a", "b", "c"],
                "pd": [0.2, 0.3, 0.1], "importance": 0.2}],
           "pairs": [{"i": 0, "j": 1, "zi": [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4], [0.3, 0.5, 0.9]]},
                     {"i": 0, "j": 2, "zi": [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4], [0.3, 0.5, 0.9]]},
                     {"i": 1, "j": 2, "zi": [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4], [0.3, 0.5, 0.9]]}]}
    path = tmp_path / "objective.png"
    analysis.plot_report(rep, str(path))
    data = path.read_bytes()
    assert len(data) > 1000 and data[:8] == b"\x89PNG\r\n\x1a\n"
    with pytest.raises(ValueError):
        analysis.plot_report({"best_observed": None, "model": None}, str(tmp_path / "none.png"))
