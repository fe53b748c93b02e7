"""Host side of the joint posterior and the Thompson batch (no GPU): the refusals of
``mpo_gp_joint_ws_bytes`` / ``mpo_gp_posterior_cov`` / ``mpo_gp_sample`` on host structs
(every check runs before any launch), the ``batch_strategy`` keyword through the
optimizer's configuration, pickles, ``ChainJob`` and the CLI, the dedupe rule and the
jitter ladder on a stubbed ``DeviceGP.sample``."""
import ctypes
import pickle

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import STRATEGIES, ChainJob, GPModel, Optimizer
from mpi_opt_amd.search import make_parser

MPO_EINVAL, MPO_ENOTSUP = 1, 3
SPACE = [(0.0, 1.0), (0.0, 1.0)]


@pytest.fixture
def buf():
    b = ctypes.create_string_buffer(64)
    yield ctypes.addressof(b)
    del b


def model(n, p=None, d=10, dp=12):
    """A host struct with the shape fields set and every pointer the joint kernels follow
    aimed at ``p`` (never dereferenced: the calls below are all refused on the host)."""
    return _lib.MpoGpModel(n=n, d=d, dp=dp, np16=(n + 15) // 16 * 16, amp=1.0, y_std=1.0, xs=p, ls=p, alpha=p, W=p)


def cov(md, p, m, ldc=None, ws_bytes=1 << 40, cand=True, out=True, ws=True):
    L = _lib.lib()
    rc = L.mpo_gp_posterior_cov(ctypes.byref(md) if md is not None else None, p if cand else None, m, None,
                                p if out else None, m if ldc is None else ldc, p if ws else None, ws_bytes, None)
    return rc, L.mpo_last_error()


def sample(md, p, m, s, jitter=1e-8, ws_bytes=1 << 40, cand=True, z=True, info=True, ws=True):
    L = _lib.lib()
    rc = L.mpo_gp_sample(ctypes.byref(md) if md is not None else None, p if cand else None, m, p if z else None, s,
                         jitter, None, None, p if info else None, p if ws else None, ws_bytes, None)
    return rc, L.mpo_last_error()


def test_joint_ws_bytes_limits():
    L = _lib.lib()
    md = model(200)
    assert _lib.MPO_JOINT_MAX == 4096
    cov_only = L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 4096, 0)
    assert cov_only >= 4096 * 208 * 8
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 4096, 256) >= cov_only + 4096 * 4096 * 8
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 1, 1) > 0
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 4097, 0) == 0
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 0, 0) == 0
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 16, -1) == 0
    assert L.mpo_gp_joint_ws_bytes(None, 16, 1) == 0
    big, last = model(2049), model(2048)
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(big), 16, 1) == 0
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(last), 16, 1) > 0
    bad = model(200, dp=10)                                          # dp is never 10
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(bad), 16, 1) == 0


def test_posterior_cov_refusals(buf):
    md = model(200, buf)
    assert cov(None, buf, 16)[0] == MPO_EINVAL
    rc, msg = cov(md, buf, 16, cand=False)
    assert rc == MPO_EINVAL and b"null" in msg
    assert cov(md, buf, 16, out=False)[0] == MPO_EINVAL
    assert cov(md, buf, 16, ws=False)[0] == MPO_EINVAL
    assert cov(md, buf, 0)[0] == MPO_EINVAL
    assert cov(md, buf, 16, ldc=15)[0] == MPO_EINVAL
    assert cov(model(200), buf, 16)[0] == MPO_EINVAL                  # no factor behind the struct
    assert cov(model(0, buf), buf, 16)[0] == MPO_EINVAL
    assert cov(model(200, buf, dp=10), buf, 16)[0] == MPO_EINVAL
    need = _lib.lib().mpo_gp_joint_ws_bytes(ctypes.byref(md), 16, 0)
    rc, msg = cov(md, buf, 16, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    rc, msg = cov(md, buf, 4097)
    assert rc == MPO_ENOTSUP and b"4096" in msg
    rc, msg = cov(model(2049, buf), buf, 16)
    assert rc == MPO_ENOTSUP and b"2048" in msg


def test_sample_refusals(buf):
    md = model(200, buf)
    assert sample(None, buf, 16, 4)[0] == MPO_EINVAL
    for null in ("cand", "z", "info", "ws"):
        rc, msg = sample(md, buf, 16, 4, **{null: False})
        assert rc == MPO_EINVAL and b"null" in msg, null
    assert sample(md, buf, 0, 4)[0] == MPO_EINVAL
    assert sample(md, buf, 16, 0)[0] == MPO_EINVAL
    for jitter in (-1e-12, float("nan"), float("inf")):
        rc, msg = sample(md, buf, 16, 4, jitter=jitter)
        assert rc == MPO_EINVAL and b"jitter" in msg
    assert sample(model(200), buf, 16, 4)[0] == MPO_EINVAL
    need = _lib.lib().mpo_gp_joint_ws_bytes(ctypes.byref(md), 16, 4)
    rc, msg = sample(md, buf, 16, 4, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    # the covariance-only size does not serve a sampling call
    assert sample(md, buf, 16, 4, ws_bytes=_lib.lib().mpo_gp_joint_ws_bytes(ctypes.byref(md), 16, 0))[0] == MPO_EINVAL
    assert sample(md, buf, 4097, 4)[0] == MPO_ENOTSUP
    assert sample(model(2049, buf), buf, 16, 4)[0] == MPO_ENOTSUP


def test_header_says_sampling_is_not_the_reference():
    import os
    import re

    from tests.conftest import ROOT

    src = open(os.path.join(ROOT, "include", "mpo.h")).read()
    comment = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int mpo_gp_sample\(", src, flags=re.S)
    assert comment and "NOT the reference's semantics" in comment[0]


# ---- batch_strategy through the optimizer ------------------------------------------------
def test_strategies_keep_their_index():
    assert STRATEGIES[:3] == ("cl_min", "cl_mean", "cl_max") and STRATEGIES[-1] == "thompson"
    assert STRATEGIES.index("cl_min") == 0


def test_batch_strategy_values():
    assert Optimizer(SPACE, random_state=0).batch_strategy == "cl_min"
    assert Optimizer(SPACE, random_state=0, batch_strategy="thompson").batch_strategy == "thompson"
    for bad in ("ts", None, "Thompson", 0):
        with pytest.raises(ValueError, match="batch_strategy"):
            Optimizer(SPACE, random_state=0, batch_strategy=bad)
    opt = Optimizer(SPACE, random_state=0)
    with pytest.raises(ValueError, match="strategy"):
        opt.ask(2, strategy="cl_median")
    with pytest.raises(ValueError, match="strategy"):
        opt.ask(2, "ts")


def test_config_copy_pickle_keep_thompson():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4, batch_strategy="thompson")
    assert opt._config()["batch_strategy"] == "thompson"
    opt.tell([0.2, 0.3], 1.0)                       # inside the initial points: no GP, no device
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "thompson")))
    assert job.config["batch_strategy"] == "thompson" and job.strategy == "thompson"
    assert job.copy_optimizer().batch_strategy == "thompson"
    assert opt.copy(random_state=3).batch_strategy == "thompson"
    assert pickle.loads(pickle.dumps(opt)).batch_strategy == "thompson"
    assert Optimizer(SPACE, random_state=0).copy(random_state=3).batch_strategy == "cl_min"


def test_old_pickle_loads_as_cl_min():
    opt = Optimizer(SPACE, random_state=0)
    state = opt.__getstate__()
    del state["batch_strategy"]                     # a checkpoint written before the keyword existed
    old = Optimizer.__new__(Optimizer)
    old.__setstate__(state)
    assert old.batch_strategy == "cl_min" and old._config()["batch_strategy"] == "cl_min"


def test_chain_job_encode_decode_keeps_the_strategy_and_its_cost():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4)
    opt.tell([[0.2, 0.3], [0.4, 0.1]], [1.0, 2.0])
    for strategy in STRATEGIES:
        job = ChainJob(opt, 11, 5, strategy)
        meta, blob = job.encode()
        assert int(meta[6]) == STRATEGIES.index(strategy)
        back = ChainJob.decode(meta, blob, opt._config())
        assert back.strategy == strategy and back.cost == job.cost and back.Xi == job.Xi
    assert int(ChainJob(opt, 11, 5, "cl_min").encode()[0][6]) == 0
    assert ChainJob(opt, 11, 5, "thompson").cost == 3.0 ** 2                  # one refit, (n0 + 1)^2
    assert ChainJob(opt, 11, 5, "cl_min").cost == sum((2 + i + 1) ** 2 for i in range(5))


def test_thompson_batch_inside_the_initial_points_is_the_cl_min_batch():
    """No model is needed while the copy still has initial points: the batch is cl_min's."""
    a = Optimizer(SPACE, random_state=5, n_initial_points=6)
    b = Optimizer(SPACE, random_state=5, n_initial_points=6)
    c = Optimizer(SPACE, random_state=5, n_initial_points=6, batch_strategy="thompson")
    ref = a.ask(3, "cl_min")
    assert b.ask(3, "thompson") == ref and c.ask(3) == ref
    assert len(b.yi) == 0 and list(b.cache_) == [(3, "thompson")]


def test_too_many_thompson_candidates_is_a_value_error():
    opt = Optimizer(SPACE, random_state=0, acq_optimizer_kwargs={"n_ts_points": 4097})
    with pytest.raises(ValueError, match="n_ts_points"):
        opt.ask(2, "thompson")


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).batch_strategy == "cl_min"
    assert p.parse_args(["--batch-strategy", "thompson"]).batch_strategy == "thompson"
    with pytest.raises(SystemExit):
        p.parse_args(["--batch-strategy", "cl_max"])
    flag = next(a for a in p._actions if "--batch-strategy" in a.option_strings)
    assert "NOT the reference" in flag.help


# ---- dedupe and the jitter ladder ---------------------------------------------------------
def test_dedupe_takes_the_lowest_free_sample_in_draw_order():
    S = np.array([[3.0, 1.0, 2.0, 5.0],
                  [9.0, 0.0, 4.0, 4.0],      # collides with draw 0 on 1; ties 2 / 3 -> lowest index
                  [0.5, 7.0, 8.0, 9.0],
                  [6.0, 0.1, 0.2, 0.3]])     # 1 and 2 taken -> 3
    fetched = []

    def row_of(k):
        fetched.append(k)
        return S[k]

    picks = OPT.thompson_dedupe(np.argmin(S, axis=1), row_of)
    assert picks == [1, 2, 0, 3] and fetched == [1, 3]
    assert S[1, 2] == 4.0                                            # the caller's rows are not written


class _StubDev:
    """DeviceGP.sample that fails its factorisation ``fails`` times."""

    def __init__(self, fails):
        self.fails, self.jitters = fails, []

    def sample(self, cand, z, jitter=1e-8, want_samples=True):
        self.jitters.append(jitter)
        bad = len(self.jitters) <= self.fails
        import torch

        z = np.asarray(z)
        return {"samples": torch.from_numpy(np.ascontiguousarray(z.T) * jitter), "argmin": None,
                "info": 7 if bad else 0}


def test_jitter_ladder_on_a_stubbed_device():
    est = GPModel(np.zeros((3, 2)), np.arange(3.0), 1.0, np.ones(2), 0.1)
    est._dev = _StubDev(fails=2)
    out = est.sample_y(np.zeros((5, 2)), n_samples=4, random_state=3)
    assert est._dev.jitters == [1e-8, 1e-6, 1e-4]
    z = np.random.RandomState(3).standard_normal((5, 4))
    assert out.shape == (5, 4) and np.array_equal(out, z * 1e-4)
    est._dev = _StubDev(fails=0)
    est.sample_y(np.zeros((5, 2)))
    assert est._dev.jitters == [1e-8]
    est._dev = _StubDev(fails=3)
    with pytest.raises(np.linalg.LinAlgError, match="column 6"):
        est.sample_y(np.zeros((5, 2)))
    assert est._dev.jitters == [1e-8, 1e-6, 1e-4]
    assert OPT.JITTER_LADDER == (1e-8, 1e-6, 1e-4)


def test_gp_model_predict_refuses_std_and_cov_together():
    est = GPModel(np.zeros((3, 2)), np.arange(3.0), 1.0, np.ones(2), 0.1)
    with pytest.raises(RuntimeError):
        est.predict(np.zeros((2, 2)), return_std=True, return_cov=True)
