"""Host side of the device candidate source (no GPU): the numpy yardstick
(tests/philox_ref.py) against the Random123 known-answer vectors and the transformed
grid, ``mpo_space_sample``'s refusals before any GPU call, and the ``candidates`` keyword
through the optimizer's configuration, pickles, chain jobs and the CLI."""
import ctypes
import pickle

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd.candidates import dim_table
from mpi_opt_amd.models import mnist_space
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from mpi_opt_amd.search import make_parser
from mpi_opt_amd.space import Categorical, Integer, Real, Space
from tests import philox_ref as P

MPO_EINVAL = 1
SPACE = [(0.0, 1.0), (0.0, 1.0)]
R, I, C = _lib.MPO_DIM_REAL, _lib.MPO_DIM_INTEGER, _lib.MPO_DIM_CATEGORICAL


@pytest.mark.parametrize("counter, key, expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    out = P.philox4x32_10(counter, key)
    assert " ".join(f"{int(v):08x}" for v in out) == expect
    # the vectorised form gives every lane the scalar answer
    lanes = P.philox4x32_10([np.full(3, c) for c in counter], key)
    assert all(np.all(lane == v) for lane, v in zip(lanes, out))


def test_u53_range_and_resolution():
    assert P.u53(0, 0) == 0.0
    assert P.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert P.u53(0, 1 << 6) == 2.0 ** -53 and P.u53(1 << 5, 0) == 2.0 ** -27
    assert P.u53(0x1F, 0x3F) == 0.0                     # the dropped low bits


def test_integer_columns_lie_on_the_transform_grid():
    dims = mnist_space()
    X = P.sample_transformed(dims, 5000, seed=77)
    assert X.shape == (5000, 5) and X.dtype == np.float64
    for j, dim in enumerate(dims[:4]):
        grid = dim.transform(np.arange(dim.low, dim.high + 1))
        assert np.isin(X[:, j], grid).all()
        assert set(np.unique(X[:, j])) == set(grid)    # 5000 draws reach every value, the ends too
        back = dim.inverse_transform(X[:, j])
        assert np.array_equal(dim.transform(back), X[:, j])
    assert (X[:, 4] >= 0).all() and (X[:, 4] < 1).all()
    # the end values carry half the mass of an inner one (skopt's round of a uniform draw)
    k = np.rint(X[:, 1] * 8)
    assert 0.3 < np.mean(k == 0) / np.mean(k == 4) < 0.7


def test_one_hot_rows_and_small_categoricals():
    dims = [Categorical("abc"), Categorical("ab"), Categorical("a"), Integer(4, 4), Categorical(list(range(7)))]
    X = P.sample_transformed(dims, 2000, seed=3, first=10)
    assert X.shape == (2000, 3 + 1 + 1 + 1 + 7) == (2000, Space(dims).transformed_n_dims)
    for block in (X[:, :3], X[:, 6:]):
        assert np.isin(block, (0.0, 1.0)).all() and (block.sum(axis=1) == 1.0).all()
        assert (block.sum(axis=0) > 0).all()
    assert set(np.unique(X[:, 3])) == {0.0, 1.0}
    assert not X[:, 4].any() and not X[:, 5].any()
    # rows are a function of (seed, index): a slice is the same rows
    assert np.array_equal(P.sample_transformed(dims, 5, seed=3, first=12), X[2:7])


def test_dim_table():
    dims = [Real(1e-3, 1.0, prior="log-uniform"), Integer(3, 9), Categorical("abcd"), Categorical("ab"), (0, 1)]
    table, d = dim_table(Space(dims))
    assert d == 1 + 1 + 4 + 1 + 1 and len(table) == 5
    assert [(t.kind, t.count) for t in table] == [(R, 0), (I, 6), (C, 4), (C, 2), (I, 1)]
    assert ctypes.sizeof(_lib.MpoDimDesc) == 16


def sample(dims, d, first=0, m=4, out=True, n_dims=None):
    table = (_lib.MpoDimDesc * max(len(dims), 1))()
    for t, (kind, count) in zip(table, dims):
        t.kind, t.count = kind, count
    buf = ctypes.create_string_buffer(64)               # never written: every call here is refused
    rc = _lib.lib().mpo_space_sample(table, len(dims) if n_dims is None else n_dims, d, 1, first, m,
                                     ctypes.addressof(buf) if out else None, None)
    return rc, _lib.lib().mpo_last_error()


def test_sample_refuses_bad_arguments_without_a_gpu():
    ok = [(R, 0), (I, 3)]
    rc, msg = sample(ok, 2, out=False)
    assert rc == MPO_EINVAL and b"null output" in msg
    assert _lib.lib().mpo_space_sample(None, 2, 2, 1, 0, 4, None, None) == MPO_EINVAL
    for n_dims in (0, 33, -1):
        rc, msg = sample([(R, 0)] * 33, 2, n_dims=n_dims)
        assert rc == MPO_EINVAL and b"n_dims" in msg
    rc, msg = sample(ok, 3)
    assert rc == MPO_EINVAL and b"2 transformed columns" in msg
    assert sample([(R, 0), (C, 3)], 2)[0] == MPO_EINVAL                      # the one-hot block takes 3
    assert sample([(R, 0)] * 20 + [(C, 13)], 33)[0] == MPO_EINVAL            # d > 32
    assert sample([(R, 0)] * 20 + [(C, 13)], 32)[0] == MPO_EINVAL            # width 33, whatever d says
    assert sample(ok, 0)[0] == MPO_EINVAL
    rc, msg = sample([(R, 0), (7, 0)], 2)
    assert rc == MPO_EINVAL and b"unknown kind" in msg
    rc, msg = sample([(C, 0)], 1)
    assert rc == MPO_EINVAL and b"Categorical" in msg
    rc, msg = sample([(I, -1)], 1)
    assert rc == MPO_EINVAL and b"Integer span" in msg
    assert sample([(I, 1 << 52)], 1)[0] == MPO_EINVAL
    for first, m in ((0, -1), (-1, 4)):
        rc, msg = sample(ok, 2, first=first, m=m)
        assert rc == MPO_EINVAL and b"negative" in msg
    rc, msg = sample(ok, 2, first=(1 << 62) - 3, m=4)
    assert rc == MPO_EINVAL and b"2^62" in msg
    with pytest.raises(_lib.MpoError, match="unknown kind"):
        _lib.check(sample([(9, 0)], 1)[0], "mpo_space_sample")


def test_sample_of_no_rows_succeeds_and_launches_nothing():
    assert sample([(R, 0), (I, 3)], 2, m=0, out=False)[0] == 0
    assert sample([(R, 0), (I, 3)], 2, first=1 << 62, m=0, out=False)[0] == 0
    assert sample([(R, 0), (I, 3)], 3, m=0, out=False)[0] == MPO_EINVAL      # still validated


def test_candidates_values():
    assert Optimizer(SPACE, random_state=0).candidates == "host"
    assert Optimizer(SPACE, random_state=0, candidates="device").candidates == "device"
    for bad in ("bogus", None, "Device", 0):
        with pytest.raises(ValueError, match="candidates"):
            Optimizer(SPACE, random_state=0, candidates=bad)


def test_old_pickle_loads_as_host():
    opt = Optimizer(SPACE, random_state=0)
    state = opt.__getstate__()
    del state["candidates"]                         # a checkpoint written before the keyword existed
    old = Optimizer.__new__(Optimizer)
    old.__setstate__(state)
    assert old.candidates == "host" and old._config()["candidates"] == "host"


def test_config_and_chain_job_keep_device():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4, candidates="device")
    assert opt._config()["candidates"] == "device"
    assert Optimizer(SPACE, random_state=0)._config()["candidates"] == "host"
    opt.tell([0.2, 0.3], 1.0)                       # inside the initial points: no GP, no device
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "cl_min")))
    assert job.config["candidates"] == "device"
    assert job.copy_optimizer().candidates == "device"
    meta, blob = ChainJob(opt, 7, 2, "cl_min").encode()
    back = ChainJob.decode(meta, blob, opt._config())
    copy = back.copy_optimizer()
    assert copy.candidates == "device" and copy.Xi == [[0.2, 0.3]] and back.seed == 7
    assert opt.copy(random_state=3).candidates == "device"
    assert pickle.loads(pickle.dumps(opt)).candidates == "device"
    assert Optimizer(SPACE, random_state=0).copy(random_state=3).candidates == "host"


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).candidate_source == "host"
    assert p.parse_args(["--candidate-source", "device"]).candidate_source == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--candidate-source", "gpu"])
    flag = next(a for a in p._actions if "--candidate-source" in a.option_strings)
    assert "NOT the reference" in flag.help
