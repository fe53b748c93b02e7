"""CPU checks of the pathwise polish (``mpo_gp_paths_grad``, ``ts_polish``): the numpy
restatement against itself (tests/paths_grad_ref.py), the host-side refusals of the device
entry point, the fallback rule, ``thompson_config``, the CLI flag and the key's way through
copies and chain jobs.  No GPU.
"""
import ctypes
import pickle

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from mpi_opt_amd.search import main, make_parser
from tests import paths_grad_ref as G
from tests import paths_ref as R
from tests.test_gp_paths_host import buf, model, paths_of  # noqa: F401  (buf is a fixture)

MPO_EINVAL = 1
SPACE = [(0.0, 1.0), (0.0, 1.0)]


# ---- the restatement alone ---------------------------------------------------------------------
def test_restated_gradient_is_the_derivative_of_the_restated_value():
    """fp64, central differences with h = 1e-6 on PATH_CASE: within 1e-6 max|g| (measured
    9.6e-9 at max|g| 2.5 when the issue was written; the margin covers eps / h elsewhere)."""
    X, y, C, (amp, ls, noise), rnd = R.path_case()
    d, s = X.shape[1], rnd[2].shape[1]
    draws = np.arange(len(C)) % s
    coef = G.coefficients(X, y, amp, ls, noise, *rnd, precision="fp64")
    vg = lambda P: G.value_grad(X, y, P, draws, amp, ls, noise, *rnd, precision="fp64", coef=coef)  # noqa: E731
    _, g, _ = vg(C)
    h, num = 1e-6, np.empty_like(g)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        num[:, k] = (vg(C + e)[0] - vg(C - e)[0]) / (2 * h)
    err, top = float(np.max(np.abs(num - g))), float(np.max(np.abs(g)))
    print(f"max |central difference - g| {err:.3e} at max|g| {top:.3g}")
    assert err <= 1e-6 * top


def test_fp64_restatement_is_within_the_reference_bar_of_80_bits():
    X, y, C, (amp, ls, noise), rnd = R.path_case()
    draws = np.arange(len(C)) % rnd[2].shape[1]
    P = np.vstack([C, X[:1], np.ones((1, X.shape[1]))])      # plus a point on an observation and a corner
    draws = np.concatenate([draws, [0, 1]])
    fx, gx, gs = G.value_grad(X, y, P, draws, amp, ls, noise, *rnd, precision="exact")
    f64, g64, _ = G.value_grad(X, y, P, draws, amp, ls, noise, *rnd, precision="fp64")
    scale = R.normalise(y)[1] * np.sqrt(amp)
    ef = float(np.max(np.abs(f64 - fx))) / scale
    eg = float(np.max(np.abs(g64 - gx) / gs))
    print(f"fp64 vs 80-bit: f {ef:.3e} of y_std sqrt(amp), g {eg:.3e} of its summand scale")
    assert ef <= R.REF_BAR and eg <= R.REF_BAR


# ---- host-side refusals of the device form (nothing is launched) -----------------------------------
def grad(md, pt, p, batch, null=None, host=False):
    L = _lib.lib()
    a = {k: p for k in ("x", "draw", "f", "g")}
    if null in a:
        a[null] = None
    fn = L.mpo_gp_paths_grad_host if host else L.mpo_gp_paths_grad
    rc = fn(ctypes.byref(md) if md is not None else None, ctypes.byref(pt) if pt is not None else None, a["x"],
            a["draw"], batch, a["f"], a["g"], None)
    return rc, L.mpo_last_error()


def test_grad_refusals_on_the_host(buf):  # noqa: F811
    assert _lib.MPO_PATHS_GRAD_BMAX == 8192
    md, pt = model(200, buf), paths_of(200, 64, 32, buf)
    for host in (False, True):
        assert grad(None, pt, buf, 4, host=host)[0] == MPO_EINVAL
        assert grad(md, None, buf, 4, host=host)[0] == MPO_EINVAL
        for null in ("x", "draw", "f", "g"):
            rc, msg = grad(md, pt, buf, 4, null=null, host=host)
            assert rc == MPO_EINVAL and b"null" in msg, null
        for batch in (0, -1, 8193):
            rc, msg = grad(md, pt, buf, batch, host=host)
            assert rc == MPO_EINVAL and b"batch" in msg, batch
        assert grad(model(200), pt, buf, 4, host=host)[0] == MPO_EINVAL                  # no factor behind the struct
        assert grad(model(200, buf, dp=20), paths_of(200, 64, 32, buf, dp=20), buf, 4, host=host)[0] == MPO_EINVAL
        assert grad(model(2049, buf), paths_of(2049, 64, 32, buf), buf, 4, host=host)[0] == MPO_EINVAL
        rc, msg = grad(model(201, buf), pt, buf, 4, host=host)                           # paths of another model
        assert rc == MPO_EINVAL and b"malformed paths" in msg
        bad = paths_of(200, 64, 32, buf)
        bad.sp -= 16
        assert grad(md, bad, buf, 4, host=host)[0] == MPO_EINVAL
        assert grad(md, paths_of(200, 64, 32, None), buf, 4, host=host)[0] == MPO_EINVAL  # no coefficients


def test_header_says_the_polish_is_not_the_reference():
    import os

    from tests.conftest import ROOT

    src = open(os.path.join(ROOT, "include", "mpo.h")).read()
    block = src[src.index("Value and gradient of draw[b]"):src.index("int mpo_gp_paths_grad_host")]
    assert "NOT the reference's semantics" in block and "MPO_PATHS_GRAD_BMAX 8192" in block
    block = src[src.index("Each draw of a set of sample paths"):src.index("int mpo_gp_paths_polish_host")]
    assert "NOT the reference's" in block


# ---- the fallback rule ---------------------------------------------------------------------------
def test_polished_points_fall_back_to_their_candidates_when_they_repeat():
    acc = OPT.thompson_polish_accept
    pol = [[0.5, 1], [0.25, 2], [0.5, 1], [0.5, 1], [0.75, 3], [0.1, 0]]
    cand = [[0.4, 1], [0.2, 2], [0.6, 1], [0.75, 3], [0.7, 3], [0.1, 0]]
    pts, kept = acc(pol, cand)
    # draws 2 and 3 repeat draw 0 and take their candidates; draw 4's polished point repeats draw
    # 3's accepted candidate and falls back too
    assert kept == [True, True, False, False, False, True]
    assert pts == [[0.5, 1], [0.25, 2], [0.6, 1], [0.75, 3], [0.7, 3], [0.1, 0]]
    assert acc([], []) == ([], [])
    assert acc([[1, "a"]], [[2, "b"]]) == ([[1, "a"]], [True])
    # numpy scalars and python numbers that compare equal are the same point
    pts, kept = acc([[np.float64(0.5), np.int64(1)], [0.5, 1]], [[0.0, 0], [0.3, 1]])
    assert kept == [True, False] and pts[1] == [0.3, 1]
    # the inputs are not written
    assert pol[2] == [0.5, 1] and cand[2] == [0.6, 1]


# ---- ts_polish through the optimizer ----------------------------------------------------------------
KW = {"ts_sampler": "paths", "n_ts_features": 512, "n_ts_points": 5000, "ts_polish": True}


def test_thompson_config_refusals_and_its_unchanged_tuple():
    cfg = OPT.thompson_config
    assert cfg({"ts_sampler": "paths", "ts_polish": True}, 10000, 4) == ("paths", 10000, 2048)
    assert cfg({"ts_sampler": "paths", "ts_polish": False}, 10000, 4) == ("paths", 10000, 2048)
    assert cfg({"ts_polish": False}, 10000, 4) == ("joint", 2048, 2048)
    assert cfg({"ts_sampler": "joint", "ts_polish": False}, 10000, 4) == ("joint", 2048, 2048)
    assert cfg({"ts_sampler": "paths", "ts_polish": np.True_}, 10000, 4) == ("paths", 10000, 2048)
    for kw in ({"ts_polish": True}, {"ts_sampler": "joint", "ts_polish": True}):
        with pytest.raises(ValueError, match="ts_polish.*paths"):
            cfg(kw, 10000, 4)
    for bad in (1, 0, "yes", "", None, 1.0, [True]):
        for sampler in ("joint", "paths"):
            with pytest.raises(ValueError, match="ts_polish.*bool"):
                cfg({"ts_sampler": sampler, "ts_polish": bad}, 10000, 4)
    # the limits of the sampler still hold under the key
    with pytest.raises(ValueError, match="n_ts_features"):
        cfg({"ts_sampler": "paths", "ts_polish": True, "n_ts_features": 4097}, 10000, 4)
    with pytest.raises(ValueError, match="1024"):
        cfg({"ts_sampler": "paths", "ts_polish": True}, 10000, 1025)


@pytest.mark.parametrize("kw,match", [({"ts_polish": True}, "ts_polish"),
                                      ({"ts_sampler": "joint", "ts_polish": True}, "ts_polish"),
                                      ({"ts_sampler": "paths", "ts_polish": "on"}, "bool"),
                                      ({"ts_sampler": "paths", "ts_polish": 1}, "bool")])
def test_ask_refuses_before_any_fit(kw, match, monkeypatch):
    def no_fit(*a, **k):
        raise AssertionError("a fit ran before the refusal")

    monkeypatch.setattr(OPT, "fit_gp_hyperparameters", no_fit)
    opt = Optimizer(SPACE, random_state=0, n_initial_points=10, acq_optimizer_kwargs=kw)
    with pytest.raises(ValueError, match=match):
        opt.ask(12, "thompson")
    assert not opt.models and opt.cache_ == {}


def test_config_copy_pickle_chainjob_keep_the_key():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4, batch_strategy="thompson", acq_optimizer_kwargs=KW)
    assert opt._config()["acq_optimizer_kwargs"]["ts_polish"] is True
    assert opt.copy(random_state=3).acq_optimizer_kwargs["ts_polish"] is True
    assert pickle.loads(pickle.dumps(opt)).acq_optimizer_kwargs["ts_polish"] is True
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "thompson")))
    assert job.config["acq_optimizer_kwargs"] == KW
    meta, blob = ChainJob(opt, 7, 2, "thompson").encode()
    back = ChainJob.decode(meta, blob, opt._config())
    assert back.strategy == "thompson" and back.copy_optimizer().acq_optimizer_kwargs == KW


def test_cli_flag_and_its_refusal(capsys):
    p = make_parser()
    assert p.parse_args([]).thompson_polish is False
    ok = ["--batch-strategy", "thompson", "--thompson-sampler", "paths", "--thompson-polish"]
    assert p.parse_args(ok).thompson_polish is True
    flag = next(a for a in p._actions if "--thompson-polish" in a.option_strings)
    assert "NOT the reference's semantics" in flag.help and flag.default is False
    for argv in (["--thompson-polish"], ["--thompson-polish", "--batch-strategy", "thompson"],
                 ["--thompson-polish", "--thompson-sampler", "paths"],
                 ["--thompson-polish", "--batch-strategy", "thompson", "--thompson-sampler", "joint"]):
        assert main(argv) == 2, argv
        assert "--thompson-polish needs" in capsys.readouterr().err
