"""Host side of the pathwise posterior samples (no GPU): the law of ``draw_paths``, the moments
of the fp64 restatement (tests/paths_ref.py), the refusals of the four ``mpo_gp_paths_*`` entry
points on host structs (every check runs before any launch), and the ``ts_sampler`` /
``n_ts_features`` keys through the optimizer's configuration, pickles, ``ChainJob`` and the CLI."""
import ctypes
import pickle

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from mpi_opt_amd.paths import draw_paths
from mpi_opt_amd.search import make_parser
from oracle import gp_ei as O
from tests import joint_cases as J
from tests import paths_ref as R

MPO_EINVAL, MPO_ENOTSUP = 1, 3
SPACE = [(0.0, 1.0), (0.0, 1.0)]


# ---- the law ---------------------------------------------------------------------------------
def test_draw_paths_is_the_restated_one_bit_for_bit():
    a = draw_paths(np.random.RandomState(7), 33, 5, 4, 9)
    b = R.draw_paths(np.random.RandomState(7), 33, 5, 4, 9)
    assert [x.shape for x in a] == [(33, 5), (33,), (33, 4), (9, 4)]
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # the order of the draws: the normals of omega first, then chi^2, the phases, w, eps
    rs = np.random.RandomState(7)
    z, u, ph = rs.standard_normal((33, 5)), rs.chisquare(5, 33), rs.uniform(0.0, 2.0 * np.pi, 33)
    assert np.array_equal(a[0], z * np.sqrt(5.0 / u)[:, None]) and np.array_equal(a[1], ph)
    assert np.array_equal(a[2], rs.standard_normal((33, 4))) and np.array_equal(a[3], rs.standard_normal((9, 4)))
    assert np.all((a[1] >= 0.0) & (a[1] < 2.0 * np.pi))


def test_frequencies_follow_the_matern52_spectral_law():
    """E cos(omega . r) = Matern52(|r|) at unit length scale (Bochner)."""
    omega = draw_paths(np.random.RandomState(0), 400000, 3, 1, 1)[0]
    for r in (0.1, 0.5, 1.0, 2.0):
        vec = np.array([r, 0.0, 0.0])
        got, want = float(np.mean(np.cos(omega @ vec))), float(R.matern52_unit(r))
        print(f"r = {r}: mean cos {got:.5f}, Matern52 {want:.5f}, diff {abs(got - want):.2e}")
        assert abs(got - want) <= 1e-2


def test_moments_of_the_restatement_match_the_posterior():
    """4000 draws at F = 2048: the sample mean within 0.15 exact posterior sd at every point,
    the sample sd within [0.85, 1.25] of it (the prior is approximated)."""
    n, d, m, F, s = 64, 4, 96, 2048, 4000
    X, y, C, _ = J.inputs(n, d, m)
    amp, ls, noise = J.theta(d)
    S, _ = R.samples(X, y, C, amp, ls, noise, *draw_paths(np.random.RandomState(5), F, d, s, n), precision="fp64")
    mu, sd = O.posterior_skopt(O.gp_from_theta(X, y, amp, ls, noise), C)
    e_mu = float(np.max(np.abs(S.mean(axis=0) - mu) / sd))
    ratio = S.std(axis=0) / sd
    print(f"mean within {e_mu:.3f} sd, sd ratio {ratio.min():.3f} - {ratio.max():.3f}")
    assert e_mu <= 0.15
    assert 0.85 <= ratio.min() and ratio.max() <= 1.25


# ---- refusals ----------------------------------------------------------------------------------
@pytest.fixture
def buf():
    b = ctypes.create_string_buffer(64)
    yield ctypes.addressof(b)
    del b


def model(n, p=None, d=10, dp=12):
    """A host struct with the shape fields set and every pointer the kernels follow aimed at
    ``p`` (never dereferenced: the calls below are all refused on the host)."""
    return _lib.MpoGpModel(n=n, d=d, dp=dp, np16=(n + 15) // 16 * 16, amp=1.0, y_std=1.0, xs=p, ls=p, alpha=p, W=p)


def paths_of(n, F, s, p, dp=12):
    Fp = (F + 15) // 16 * 16
    return _lib.MpoGpPaths(F=F, s=s, n=n, dp=dp, Fp=Fp, Kp=(Fp + (n + 15) // 16 * 16 + 63) // 64 * 64,
                           sp=(s + 15) // 16 * 16 + 16, omega=p, phase=p, coef=p)


def prepare(md, p, F, s, noise=0.05, ws_bytes=1 << 40, null=None):
    L = _lib.lib()
    a = {k: p for k in ("omega", "phase", "w", "eps", "ws")}
    out = _lib.MpoGpPaths()
    if null in a:
        a[null] = None
    rc = L.mpo_gp_paths_prepare(ctypes.byref(md) if md is not None else None, noise, a["omega"], a["phase"], a["w"],
                                a["eps"], F, s, None if null == "paths" else ctypes.byref(out), a["ws"], ws_bytes, None)
    return rc, L.mpo_last_error()


def evaluate(md, pt, p, m, first=0, n_draws=1, ws_bytes=1 << 40, cand=True, ws=True):
    L = _lib.lib()
    rc = L.mpo_gp_paths_eval(ctypes.byref(md) if md is not None else None,
                             ctypes.byref(pt) if pt is not None else None, p if cand else None, m, first, n_draws,
                             p, p, p, p if ws else None, ws_bytes, None)
    return rc, L.mpo_last_error()


def test_constants_and_ws_bytes_limits():
    L = _lib.lib()
    assert (_lib.MPO_PATHS_FMAX, _lib.MPO_PATHS_SMAX) == (4096, 1024)
    md = model(200)
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(md), 2048, 256) >= (2048 + 208) * 256 * 8 + 200 * 2048 * 8
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(md), 1, 1) > 0
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(md), 4096, 1024) > 0
    for F, s in ((0, 1), (1, 0), (4097, 1), (1, 1025), (-1, 4)):
        assert L.mpo_gp_paths_ws_bytes(ctypes.byref(md), F, s) == 0, (F, s)
    assert L.mpo_gp_paths_ws_bytes(None, 16, 1) == 0
    big, last = model(2049), model(2048)
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(big), 16, 1) == 0
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(last), 16, 1) > 0
    assert L.mpo_gp_paths_ws_bytes(ctypes.byref(model(200, dp=10)), 16, 1) == 0       # dp is never 10


def test_eval_ws_bytes_limits(buf):
    L = _lib.lib()
    md, pt = model(200, buf), paths_of(200, 64, 32, buf)
    q = lambda m_, p_, m, nd: L.mpo_gp_paths_eval_ws_bytes(ctypes.byref(m_) if m_ is not None else None,  # noqa: E731
                                                           ctypes.byref(p_) if p_ is not None else None, m, nd)
    assert q(md, pt, 1, 1) > 0 and q(md, pt, 10 ** 6, 32) >= 32 * 512 * 16
    assert q(md, pt, 5 * 10 ** 9, 1) > 0                                           # m is 64-bit
    for m, nd in ((0, 1), (-1, 1), (16, 0), (16, 33)):
        assert q(md, pt, m, nd) == 0, (m, nd)
    assert q(None, pt, 16, 1) == 0 and q(md, None, 16, 1) == 0
    assert q(model(201, buf), pt, 16, 1) == 0                                      # paths of another model
    bad = paths_of(200, 64, 32, buf)
    bad.Kp += 64
    assert q(md, bad, 16, 1) == 0
    assert q(model(2049, buf), paths_of(2049, 64, 32, buf), 16, 1) == 0


def test_prepare_refusals(buf):
    md = model(200, buf)
    assert prepare(None, buf, 64, 4)[0] == MPO_EINVAL
    for null in ("omega", "phase", "w", "eps", "ws", "paths"):
        rc, msg = prepare(md, buf, 64, 4, null=null)
        assert rc == MPO_EINVAL and b"null" in msg, null
    assert prepare(md, buf, 0, 4)[0] == MPO_EINVAL
    assert prepare(md, buf, 64, 0)[0] == MPO_EINVAL
    for noise in (-1e-12, float("nan"), float("inf")):
        rc, msg = prepare(md, buf, 64, 4, noise=noise)
        assert rc == MPO_EINVAL and b"noise" in msg
    assert prepare(model(200), buf, 64, 4)[0] == MPO_EINVAL                         # no factor behind the struct
    assert prepare(model(0, buf), buf, 64, 4)[0] == MPO_EINVAL
    assert prepare(model(200, buf, dp=10), buf, 64, 4)[0] == MPO_EINVAL
    need = _lib.lib().mpo_gp_paths_ws_bytes(ctypes.byref(md), 64, 4)
    rc, msg = prepare(md, buf, 64, 4, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    rc, msg = prepare(md, buf, 4097, 4)
    assert rc == MPO_ENOTSUP and b"4096" in msg
    rc, msg = prepare(md, buf, 64, 1025)
    assert rc == MPO_ENOTSUP and b"1024" in msg
    rc, msg = prepare(model(2049, buf), buf, 64, 4)
    assert rc == MPO_ENOTSUP and b"2048" in msg


def test_eval_refusals(buf):
    md, pt = model(200, buf), paths_of(200, 64, 32, buf)
    assert evaluate(None, pt, buf, 16)[0] == MPO_EINVAL
    assert evaluate(md, None, buf, 16)[0] == MPO_EINVAL
    for null in ("cand", "ws"):
        rc, msg = evaluate(md, pt, buf, 16, **{null: False})
        assert rc == MPO_EINVAL and b"null" in msg, null
    assert evaluate(md, pt, buf, 0)[0] == MPO_EINVAL
    for first, nd in ((-1, 1), (0, 0), (0, 33), (32, 1), (31, 2), (2 ** 31 - 1, 2)):
        rc, msg = evaluate(md, pt, buf, 16, first=first, n_draws=nd)
        assert rc == MPO_EINVAL and b"draws" in msg, (first, nd)
    assert evaluate(model(200), pt, buf, 16)[0] == MPO_EINVAL
    assert evaluate(md, paths_of(200, 64, 32, None), buf, 16)[0] == MPO_EINVAL      # no coefficients behind it
    assert evaluate(model(201, buf), pt, buf, 16)[0] == MPO_EINVAL                  # paths of another model
    bad = paths_of(200, 64, 32, buf)
    bad.sp -= 16
    rc, msg = evaluate(md, bad, buf, 16)
    assert rc == MPO_EINVAL and b"malformed paths" in msg
    need = _lib.lib().mpo_gp_paths_eval_ws_bytes(ctypes.byref(md), ctypes.byref(pt), 16, 4)
    rc, msg = evaluate(md, pt, buf, 16, n_draws=4, ws_bytes=need - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in msg
    assert evaluate(model(2049, buf), paths_of(2049, 64, 32, buf), buf, 16)[0] == MPO_ENOTSUP
    assert evaluate(md, paths_of(200, 4097, 32, buf), buf, 16)[0] == MPO_ENOTSUP
    assert evaluate(md, paths_of(200, 64, 1025, buf), buf, 16)[0] == MPO_ENOTSUP


def test_header_says_paths_are_not_the_reference():
    import os

    from tests.conftest import ROOT

    src = open(os.path.join(ROOT, "include", "mpo.h")).read()
    block = src[src.index("PATHWISE posterior samples"):src.index("#define MPO_PATHS_FMAX")]
    assert "NOT the reference's semantics" in block and "APPROXIMATION" in block


# ---- ts_sampler through the optimizer -----------------------------------------------------------
KW = {"ts_sampler": "paths", "n_ts_features": 512, "n_ts_points": 5000}


def test_config_copy_pickle_chainjob_keep_the_sampler():
    opt = Optimizer(SPACE, random_state=0, n_initial_points=4, batch_strategy="thompson", acq_optimizer_kwargs=KW)
    assert OPT.STRATEGIES[-1] == "thompson" and OPT.TS_SAMPLERS == ("joint", "paths")
    for k, v in KW.items():
        assert opt._config()["acq_optimizer_kwargs"][k] == v
        assert opt.copy(random_state=3).acq_optimizer_kwargs[k] == v
        assert pickle.loads(pickle.dumps(opt)).acq_optimizer_kwargs[k] == v
    job = pickle.loads(pickle.dumps(ChainJob(opt, 7, 2, "thompson")))
    assert job.config["acq_optimizer_kwargs"] == KW
    meta, blob = ChainJob(opt, 7, 2, "thompson").encode()
    back = ChainJob.decode(meta, blob, opt._config())
    assert back.strategy == "thompson" and back.copy_optimizer().acq_optimizer_kwargs == KW


def test_thompson_config_defaults_and_limits():
    cfg = OPT.thompson_config
    assert cfg({}, 10000, 4) == ("joint", 2048, 2048)
    assert cfg({"ts_sampler": "joint", "n_ts_points": 4096}, 10000, 4) == ("joint", 4096, 2048)
    assert cfg({"ts_sampler": "paths"}, 10000, 4) == ("paths", 10000, 2048)           # all n_points, no 4096 cap
    assert cfg({"ts_sampler": "paths", "n_ts_points": 10 ** 6, "n_ts_features": 4096}, 10000, 1024) == \
        ("paths", 10 ** 6, 4096)
    with pytest.raises(ValueError, match="ts_sampler"):
        cfg({"ts_sampler": "rff"}, 10000, 4)
    with pytest.raises(ValueError, match="n_ts_features"):
        cfg({"ts_sampler": "paths", "n_ts_features": 4097}, 10000, 4)
    with pytest.raises(ValueError, match="n_ts_features"):
        cfg({"ts_sampler": "paths", "n_ts_features": 0}, 10000, 4)
    with pytest.raises(ValueError, match="1024"):
        cfg({"ts_sampler": "paths"}, 10000, 1025)
    with pytest.raises(ValueError, match="n_ts_points"):
        cfg({"ts_sampler": "paths", "n_ts_points": 3}, 10000, 4)
    with pytest.raises(ValueError, match="n_ts_points"):
        cfg({"n_ts_points": 4097}, 10000, 4)


@pytest.mark.parametrize("kw,n,match", [({"ts_sampler": "paths", "n_ts_features": 4097}, 12, "n_ts_features"),
                                        ({"ts_sampler": "paths"}, 1035, "1024"),
                                        ({"ts_sampler": "paths", "n_ts_points": 3}, 14, "n_ts_points"),
                                        ({"ts_sampler": "nope"}, 12, "ts_sampler"),
                                        ({"n_ts_points": 4097}, 12, "n_ts_points"),
                                        ({"ts_sampler": "joint", "n_ts_points": 4097}, 12, "n_ts_points")])
def test_value_errors_come_before_any_fit(kw, n, match, monkeypatch):
    def no_fit(*a, **k):
        raise AssertionError("a fit ran before the refusal")

    monkeypatch.setattr(OPT, "fit_gp_hyperparameters", no_fit)
    opt = Optimizer(SPACE, random_state=0, n_initial_points=10, acq_optimizer_kwargs=kw)
    with pytest.raises(ValueError, match=match):
        opt.ask(n, "thompson")
    assert not opt.models and opt.cache_ == {}


def test_sample_paths_checks_its_sizes_before_the_device():
    est = OPT.GPModel(np.zeros((3, 2)), np.arange(3.0), 1.0, np.ones(2), 0.1)
    with pytest.raises(ValueError, match="n_features"):
        est.sample_paths(n_features=4097)
    with pytest.raises(ValueError, match="1024"):
        est.sample_paths(n_samples=1025)
    assert est._dev is None


def test_cli_flag():
    p = make_parser()
    assert p.parse_args([]).thompson_sampler == "joint"
    assert p.parse_args(["--thompson-sampler", "paths"]).thompson_sampler == "paths"
    with pytest.raises(SystemExit):
        p.parse_args(["--thompson-sampler", "rff"])
    flag = next(a for a in p._actions if "--thompson-sampler" in a.option_strings)
    assert "APPROXIMATION" in flag.help and flag.default == "joint"
