"""Host side of the fixed-theta ask batch (no GPU): ``mpo_gp_append``'s refusals on
host structs -- null pointers, a short workspace, the n = 2048 limit -- and the
``lie_refit`` keyword through the optimizer's configuration, pickles and the CLI."""
import ctypes
import pickle

import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from mpi_opt_amd.search import make_parser

MPO_EINVAL, MPO_ENOTSUP = 1, 3
SPACE = [(0.0, 1.0), (0.0, 1.0)]


def base(n, d=10, dp=12):
    return _lib.MpoGpModel(n=n, d=d, dp=dp, np16=(n + 15) // 16 * 16, amp=1.0, y_std=1.0)


def append(b, p, ws_bytes, X=True):
    m = _lib.MpoGpModel()
    rc = _lib.lib().mpo_gp_append(ctypes.byref(b) if b is not None else None, p if X else None, p, p, 0.1, 0.0, 1.0,
                                  ctypes.byref(m), p, ws_bytes, None)
    return rc, _lib.lib().mpo_last_error()


@pytest.fixture
def buf():
    b = ctypes.create_string_buffer(64)
    yield ctypes.addressof(b)
    del b


def test_null_pointers_are_invalid(buf):
    L = _lib.lib()
    assert L.mpo_gp_append(None, None, None, None, 0.1, 0.0, 1.0, None, None, 0, None) == MPO_EINVAL
    assert b"null" in L.mpo_last_error()
    assert append(None, buf, 64)[0] == MPO_EINVAL
    assert append(base(10), buf, 64, X=False)[0] == MPO_EINVAL
    b = base(10)
    assert L.mpo_gp_append(ctypes.byref(b), buf, buf, buf, 0.1, 0.0, 1.0, None, buf, 64, None) == MPO_EINVAL


def test_short_workspace_is_invalid(buf):
    need = _lib.lib().mpo_gp_prepare_ws_bytes(11, 10)
    assert need > 64
    rc, msg = append(base(10), buf, 64)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    rc, msg = append(base(10), buf, need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg


def test_malformed_base_is_invalid(buf):
    assert append(base(0), buf, 1 << 30)[0] == MPO_EINVAL
    assert append(base(10, d=10, dp=10), buf, 1 << 30)[0] == MPO_EINVAL      # dp is never 10
    rc, msg = append(base(10), buf, 1 << 30)                                 # no factor behind the struct
    assert rc == MPO_EINVAL and b"not prepared" in msg


def test_base_of_2048_is_not_supported_and_the_message_names_the_limit(buf):
    """n + 1 = 2049: refused before the workspace is looked at and before any device call."""
    rc, msg = append(base(2048), buf, 64)
    assert rc == MPO_ENOTSUP and b"2048" in msg
    assert append(base(2047), buf, 64)[0] == MPO_EINVAL                      # the last size served: only ws is short


def test_lie_refit_values():
    assert Optimizer(SPACE, random_state=0).lie_refit == "every"
    assert Optimizer(SPACE, random_state=0, lie_refit="never").lie_refit == "never"
    for bad in ("sometimes", None, "Never", 0):
        with pytest.raises(ValueError, match="lie_refit"):
            Optimizer(SPACE, random_state=0, lie_refit=bad)


def test_config_and_chain_job_keep_never():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4, lie_refit="never")
    assert opt._config()["lie_refit"] == "never"
    opt.tell([0.2, 0.3], 1.0)                       # inside the initial points: no GP, no device
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "cl_min")))
    assert job.config["lie_refit"] == "never"
    copy = job.copy_optimizer()
    assert copy.lie_refit == "never" and copy.Xi == [[0.2, 0.3]]
    assert opt.copy(random_state=3).lie_refit == "never"
    assert pickle.loads(pickle.dumps(opt)).lie_refit == "never"
    assert Optimizer(SPACE, random_state=0).copy(random_state=3).lie_refit == "every"
    # the lies of a batch that stays inside the initial points need no model in either mode
    assert len(opt.ask(2)) == 2 and len(opt.yi) == 1


def test_old_pickle_loads_as_every():
    opt = Optimizer(SPACE, random_state=0)
    state = opt.__getstate__()
    del state["lie_refit"]                          # a checkpoint written before the keyword existed
    old = Optimizer.__new__(Optimizer)
    old.__setstate__(state)
    assert old.lie_refit == "every" and old._config()["lie_refit"] == "every"


def test_stats_count_appends():
    from mpi_opt_amd import optimizer as O

    O.reset_stats()
    assert O.STATS["appends"] == 0
    O._record_refit(12, 0.0, 0.001, 0.002, 0.003, 0.006, 0.006, append=True)
    O._record_refit(13, 0.5, 0.001, 0.002, 0.003, 0.006, 0.506)
    assert (O.STATS["refits"], O.STATS["appends"], O.STATS["refit_s"]) == (2, 1, 0.5)
    O.merge_stats({"refits": 3, "appends": 2, "n_max": 40})
    assert (O.STATS["refits"], O.STATS["appends"], O.STATS["n_max"]) == (5, 3, 40)
    O.reset_stats()
    assert O.STATS["appends"] == 0 and O.STATS["refits"] == 0


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).lie_refit == "every"
    assert p.parse_args(["--lie-refit", "never"]).lie_refit == "never"
    with pytest.raises(SystemExit):
        p.parse_args(["--lie-refit", "sometimes"])
    flag = next(a for a in p._actions if "--lie-refit" in a.option_strings)
    assert "NOT the reference" in flag.help
