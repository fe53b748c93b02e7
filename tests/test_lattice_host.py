"""Host side of the lattice candidate source (no GPU): ``mpo_space_lattice_size``,
``mpo_space_lattice``'s refusals before any GPU call, the host L-BFGS-B with frozen columns
(``mpo_lbfgsb_batched_frozen``) against scipy under per-run bounds ``lo = hi = x0``, and the
``candidates="lattice"`` keyword through the optimizer's refusals, configuration, pickles,
chain jobs and the CLI."""
import ctypes
import pickle

import numpy as np
import pytest
from scipy.optimize import fmin_l_bfgs_b

from mpi_opt_amd import _lib
from mpi_opt_amd import optimizer as opt_mod
from mpi_opt_amd.candidates import SOURCES, dim_table, frozen_columns, lattice_size
from mpi_opt_amd.models import mnist_space, topclass_space
from mpi_opt_amd.optimizer import CANDIDATES, LATTICE_MAX, ChainJob, Optimizer
from mpi_opt_amd.search import make_parser
from mpi_opt_amd.space import Categorical, Integer, Real, Space

MPO_EINVAL = 1
FMIN_FTOL = 1e7 * np.finfo(float).eps
R, I, C = _lib.MPO_DIM_REAL, _lib.MPO_DIM_INTEGER, _lib.MPO_DIM_CATEGORICAL
SPACE = [Integer(0, 3), Real(0.0, 1.0), Categorical("abc")]          # L = 12, mixed
DISCRETE = [Integer(0, 6), Integer(0, 4)]                            # L = 35, nothing to polish


def table_of(dims):
    table = (_lib.MpoDimDesc * max(len(dims), 1))()
    for t, (kind, count) in zip(table, dims):
        t.kind, t.count = kind, count
    return table


def size(dims, n_dims=None):
    L = ctypes.c_int64(-7)
    rc = _lib.lib().mpo_space_lattice_size(table_of(dims), len(dims) if n_dims is None else n_dims, ctypes.byref(L))
    return rc, L.value, _lib.lib().mpo_last_error()


# ---- mpo_space_lattice_size ---------------------------------------------------------------

def test_lattice_size_of_the_search_spaces():
    assert lattice_size(mnist_space()) == 41 * 9 * 9 * 151 == 501471
    assert lattice_size(Space(mnist_space())) == 501471
    assert lattice_size(topclass_space()) == 6
    assert lattice_size([Integer(5, 5)]) == 1                                 # one value: radix 1
    assert lattice_size([Integer(0, 2), Integer(5, 5), Integer(-1, 1)]) == 9
    assert lattice_size([Real(0.0, 1.0), Real(1e-3, 1.0, prior="log-uniform")]) == 1     # no discrete dimension
    assert lattice_size([Categorical("abc"), Integer(0, 1), Categorical("ab"), Categorical("a")]) == 3 * 2 * 2 * 1
    assert size([(I, 40), (I, 8), (I, 8), (I, 150), (R, 0)])[:2] == (0, 501471)
    assert size([(I, (1 << 31) - 1), (I, (1 << 31) - 1)])[:2] == (0, 1 << 62)  # the bound itself is taken


def test_lattice_size_overflow_and_bad_tables():
    rc, _, msg = size([(I, 1 << 31), (I, (1 << 31) - 1)])                     # 2^62 + 2^31
    assert rc == MPO_EINVAL and b"2^62" in msg
    rc, _, msg = size([(I, (1 << 52) - 1)] * 2)
    assert rc == MPO_EINVAL and b"2^62" in msg
    assert size([(C, 1 << 40), (R, 0), (C, 1 << 40)])[0] == MPO_EINVAL
    with pytest.raises(_lib.MpoError, match="2\\^62"):
        lattice_size([Integer(0, 2 ** 40)] * 2)
    rc, _, msg = size([(R, 0), (7, 0)])
    assert rc == MPO_EINVAL and b"unknown kind" in msg
    assert size([(I, -1)])[0] == MPO_EINVAL and size([(C, 0)])[0] == MPO_EINVAL
    for n_dims in (0, 33, -1):
        rc, _, msg = size([(R, 0)] * 33, n_dims=n_dims)
        assert rc == MPO_EINVAL and b"n_dims" in msg
    assert _lib.lib().mpo_space_lattice_size(None, 2, ctypes.byref(ctypes.c_int64())) == MPO_EINVAL
    assert _lib.lib().mpo_space_lattice_size(table_of([(R, 0)]), 1, None) == MPO_EINVAL


# ---- mpo_space_lattice: refused, or nothing to do, before any GPU call ----------------------

def lattice(dims, d, first=0, m=4, out=True, n_dims=None, misalign=0):
    buf = ctypes.create_string_buffer(64)               # never written: every call here is refused
    rc = _lib.lib().mpo_space_lattice(table_of(dims), len(dims) if n_dims is None else n_dims, d, 1, first, m,
                                      ctypes.addressof(buf) + misalign if out else None, None)
    return rc, _lib.lib().mpo_last_error()


def test_lattice_refuses_bad_arguments_without_a_gpu():
    ok = [(R, 0), (I, 3)]
    rc, msg = lattice(ok, 2, out=False)
    assert rc == MPO_EINVAL and b"null output" in msg
    rc, msg = lattice(ok, 2, misalign=4)
    assert rc == MPO_EINVAL and b"8-byte aligned" in msg
    assert _lib.lib().mpo_space_lattice(None, 2, 2, 1, 0, 4, None, None) == MPO_EINVAL
    for n_dims in (0, 33, -1):
        rc, msg = lattice([(R, 0)] * 33, 2, n_dims=n_dims)
        assert rc == MPO_EINVAL and b"n_dims" in msg
    rc, msg = lattice(ok, 3)
    assert rc == MPO_EINVAL and b"2 transformed columns" in msg
    assert lattice([(R, 0), (C, 3)], 2)[0] == MPO_EINVAL                      # the one-hot block takes 3
    assert lattice([(R, 0)] * 20 + [(C, 13)], 33)[0] == MPO_EINVAL            # d > 32
    assert lattice([(R, 0)] * 20 + [(C, 13)], 32)[0] == MPO_EINVAL            # width 33, whatever d says
    assert lattice(ok, 0)[0] == MPO_EINVAL
    rc, msg = lattice([(R, 0), (7, 0)], 2)
    assert rc == MPO_EINVAL and b"unknown kind" in msg
    rc, msg = lattice([(C, 0)], 1)
    assert rc == MPO_EINVAL and b"Categorical" in msg
    rc, msg = lattice([(I, -1)], 1)
    assert rc == MPO_EINVAL and b"Integer span" in msg
    assert lattice([(I, 1 << 52)], 1)[0] == MPO_EINVAL
    for first, m in ((0, -1), (-1, 4)):
        rc, msg = lattice(ok, 2, first=first, m=m)
        assert rc == MPO_EINVAL and b"negative" in msg
    rc, msg = lattice(ok, 2, first=(1 << 62) - 3, m=4)
    assert rc == MPO_EINVAL and b"2^62" in msg
    rc, msg = lattice([(I, 1 << 31), (I, (1 << 31) - 1)], 2)                  # L past 2^62
    assert rc == MPO_EINVAL and b"lattice" in msg
    with pytest.raises(_lib.MpoError, match="unknown kind"):
        _lib.check(lattice([(9, 0)], 1)[0], "mpo_space_lattice")


def test_lattice_of_no_rows_succeeds_and_launches_nothing():
    assert lattice([(R, 0), (I, 3)], 2, m=0, out=False)[0] == 0
    assert lattice([(R, 0), (I, 3)], 2, first=1 << 62, m=0, out=False)[0] == 0
    assert lattice([(R, 0), (I, 3)], 3, m=0, out=False)[0] == MPO_EINVAL      # still validated
    assert lattice([(I, 1 << 31), (I, (1 << 31) - 1)], 2, m=0, out=False)[0] == MPO_EINVAL


def test_frozen_columns():
    dims = [Real(1e-3, 1.0, prior="log-uniform"), Integer(3, 9), Categorical("abcd"), Categorical("ab"), (0, 1)]
    assert frozen_columns(Space(dims)).tolist() == [False, True] + [True] * 4 + [True, True]
    assert frozen_columns(dims).dtype == bool and len(frozen_columns(dims)) == dim_table(dims)[1]
    assert frozen_columns(mnist_space()).tolist() == [True] * 4 + [False]
    assert not frozen_columns([(0.0, 1.0)] * 3).any()


# ---- the host L-BFGS-B with frozen columns ------------------------------------------------

def rosen(X):
    X = np.atleast_2d(X)
    f = np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1 - X[:, :-1]) ** 2, axis=1)
    g = np.zeros_like(X)
    g[:, :-1] += -400.0 * X[:, :-1] * (X[:, 1:] - X[:, :-1] ** 2) - 2 * (1 - X[:, :-1])
    g[:, 1:] += 200.0 * (X[:, 1:] - X[:, :-1] ** 2)
    return f, g


def native(fun, starts, bounds, frozen="plain", ftol=FMIN_FTOL):
    """``mpo_lbfgsb_batched`` (frozen="plain") or ``mpo_lbfgsb_batched_frozen`` with a mask or
    None (a null pointer): (x [R, n], f [R], stats [R, 4])."""
    L = _lib.lib()
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
    nr, n = starts.shape
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(n, 2))

    def cb(batch, X, ids, f, g, user):
        fv, gv = fun(np.ctypeslib.as_array(X, shape=(batch, n)).copy())
        np.ctypeslib.as_array(f, shape=(batch,))[:] = fv
        np.ctypeslib.as_array(g, shape=(batch, n))[:] = gv
        return 0

    cfn = _lib.FG_BATCH_FN(cb)
    opts = _lib.MpoLbfgsbOptions(ftol, 1e-5, 15000, 15000, 10, 20)
    x, f, stats, rounds = np.zeros((nr, n)), np.zeros(nr), np.zeros((nr, 4), np.int32), ctypes.c_int32(0)
    tail = (ctypes.byref(opts), cfn, None, x.ctypes.data, f.ctypes.data, stats.ctypes.data, ctypes.byref(rounds))
    if isinstance(frozen, str):
        rc = L.mpo_lbfgsb_batched(n, nr, starts.ctypes.data, b.ctypes.data, *tail)
    else:
        mask = None if frozen is None else np.ascontiguousarray(np.asarray(frozen, dtype=np.uint8))
        rc = L.mpo_lbfgsb_batched_frozen(n, nr, starts.ctypes.data, b.ctypes.data,
                                         None if mask is None else mask.ctypes.data, *tail)
    _lib.check(rc, "mpo_lbfgsb_batched_frozen")
    return x, f, stats


def test_frozen_rosenbrock_matches_scipy():
    n, box = 5, (-2.0, 2.0)
    bounds = [box] * n
    starts = np.random.RandomState(5).uniform(box[0], box[1], size=(4, n))
    starts[2, 1], starts[3, 3] = 2.75, -3.5              # outside the box on a frozen column: clipped, then held
    mask = np.zeros(n, dtype=bool)
    mask[[1, 3]] = True
    x, f, stats = native(rosen, starts, bounds, frozen=mask)
    clipped = np.clip(starts, box[0], box[1])
    assert clipped[2, 1] == 2.0 and clipped[3, 3] == -2.0
    for r in range(len(starts)):
        run_bounds = [(clipped[r, j], clipped[r, j]) if mask[j] else box for j in range(n)]
        xr, fr, info = fmin_l_bfgs_b(lambda v: tuple(a[0] for a in rosen(v[None])), starts[r], bounds=run_bounds,
                                     approx_grad=False)
        assert info["warnflag"] == 0
        assert np.max(np.abs(x[r] - xr)) <= 1e-6, (x[r], xr)
        assert abs(f[r] - fr) <= 1e-9 * max(1.0, abs(fr))
        assert x[r, mask].tobytes() == clipped[r, mask].tobytes()             # bit-equal, not close
        assert np.max(np.abs(x[r, ~mask] - clipped[r, ~mask])) > 1e-3         # the free columns did move
        assert stats[r, 2] in (1, 2)


def test_null_and_empty_masks_are_the_plain_driver():
    n, bounds = 5, [(-2.0, 0.7)] * 5
    starts = np.random.RandomState(11).uniform(-2.0, 0.7, size=(4, n))
    plain = native(rosen, starts, bounds)
    for mask in (None, np.zeros(n, dtype=bool)):
        got = native(rosen, starts, bounds, frozen=mask)
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes()


def test_all_columns_frozen_returns_the_starts():
    starts = np.array([[0.3, -1.2, 5.0], [1.0, 1.0, 1.0]])
    x, f, stats = native(rosen, starts, [(-2.0, 2.0)] * 3, frozen=[1, 1, 1])
    clipped = np.clip(starts, -2.0, 2.0)
    assert x.tobytes() == clipped.tobytes()
    assert np.array_equal(f, rosen(clipped)[0]) and (stats[:, 1] == 1).all()


# ---- Optimizer and CLI ---------------------------------------------------------------------

def test_lattice_is_an_accepted_source():
    assert "lattice" in CANDIDATES and CANDIDATES == SOURCES
    assert Optimizer(SPACE, random_state=0, candidates="lattice").candidates == "lattice"
    assert Optimizer(DISCRETE, random_state=0, candidates="lattice", acq_optimizer="sampling").candidates == "lattice"
    assert Optimizer(mnist_space(), random_state=0, candidates="lattice").candidates == "lattice"
    with pytest.raises(ValueError, match="candidates"):
        Optimizer(SPACE, random_state=0, candidates="Lattice")


def test_lattice_refusals_say_why():
    with pytest.raises(ValueError, match="lattice.*thompson"):
        Optimizer(SPACE, random_state=0, candidates="lattice", batch_strategy="thompson")
    opt = Optimizer(SPACE, random_state=0, candidates="lattice")
    with pytest.raises(ValueError, match="lattice.*thompson"):
        opt.ask(2, "thompson")
    for acq in ("EIps", "PIps"):
        with pytest.raises(ValueError, match=f"lattice.*{acq}.*polish"):
            Optimizer(SPACE, random_state=0, candidates="lattice", acq_func=acq)
    with pytest.raises(ValueError, match="lattice.*committee.*polish"):
        Optimizer(SPACE, random_state=0, candidates="lattice", surrogate="committee")
    # the same configurations are accepted by the other sources
    Optimizer(SPACE, random_state=0, candidates="device", batch_strategy="thompson")
    Optimizer(SPACE, random_state=0, candidates="device", surrogate="committee")


def test_scipy_driver_is_refused_on_a_mixed_space_only(monkeypatch):
    monkeypatch.setattr(opt_mod, "DRIVER", "scipy")
    with pytest.raises(ValueError, match="lattice.*native"):
        Optimizer(SPACE, random_state=0, candidates="lattice")
    Optimizer(DISCRETE, random_state=0, candidates="lattice")                 # nothing to polish
    Optimizer([(0.0, 1.0)] * 2, random_state=0, candidates="lattice")         # nothing to hold still
    Optimizer(SPACE, random_state=0, candidates="lattice", acq_optimizer="sampling")
    Optimizer(SPACE, random_state=0, candidates="device")


def test_lattice_max():
    assert LATTICE_MAX == 1 << 22
    big = [Integer(0, 2047), Integer(0, 2047), Real(0.0, 1.0)]                # L = 2^22: the bound itself is taken
    Optimizer(big, random_state=0, candidates="lattice")
    with pytest.raises(ValueError, match=r"L = 4196352.*lattice_max"):
        Optimizer([Integer(0, 2048), Integer(0, 2047)], random_state=0, candidates="lattice")
    with pytest.raises(ValueError, match=r"L = 501471.*lattice_max.*= 500000"):
        Optimizer(mnist_space(), random_state=0, candidates="lattice", acq_optimizer_kwargs={"lattice_max": 500000})
    Optimizer([Integer(0, 2048), Integer(0, 2047)], random_state=0, candidates="lattice",
              acq_optimizer_kwargs={"lattice_max": 1 << 23})
    Optimizer([Integer(0, 2048), Integer(0, 2047)], random_state=0, candidates="device")    # binds "lattice" only
    with pytest.raises(_lib.MpoError, match="2\\^62"):
        Optimizer([Integer(0, 2 ** 40)] * 2, random_state=0, candidates="lattice")


def test_config_and_chain_job_keep_lattice():
    kw = {"lattice_max": 64, "n_points": 100}
    space = [Integer(0, 3), Real(0.0, 1.0), Integer(-1, 1)]                   # L = 12; numbers only cross ranks
    opt = Optimizer(space, random_state=0, n_initial_points=4, candidates="lattice", acq_optimizer_kwargs=kw)
    assert opt._config()["candidates"] == "lattice"
    opt.tell([1, 0.3, -1], 1.0)                    # inside the initial points: no GP, no device
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "cl_min")))
    assert job.config["candidates"] == "lattice"
    assert job.copy_optimizer().candidates == "lattice"
    assert job.copy_optimizer().acq_optimizer_kwargs["lattice_max"] == 64
    meta, blob = ChainJob(opt, 7, 2, "cl_min").encode()
    back = ChainJob.decode(meta, blob, opt._config())
    copy = back.copy_optimizer()
    assert copy.candidates == "lattice" and copy.Xi == [[1, 0.3, -1]] and back.seed == 7
    assert opt.copy(random_state=3).candidates == "lattice"
    assert pickle.loads(pickle.dumps(opt)).candidates == "lattice"
    # a copy is refused what its asking optimizer would have been refused
    bad = dict(opt._config(), acq_optimizer_kwargs={"lattice_max": 8})
    with pytest.raises(ValueError, match="lattice_max"):
        Optimizer(random_state=1, **bad)


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).candidate_source == "host"
    assert p.parse_args(["--candidate-source", "lattice"]).candidate_source == "lattice"
    assert p.parse_args(["--candidate-source", "device"]).candidate_source == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--candidate-source", "grid"])
    flag = next(a for a in p._actions if "--candidate-source" in a.option_strings)
    assert "NOT the reference" in flag.help and "lattice" in flag.help
