"""The committee surrogate without a GPU: the reference against itself, the partition rule, the
ABI's host-side refusals on null-device structs, the workspace's independence of E, and the
optimizer's new keywords (refusals, size limits, pickles, CLI)."""
import ctypes
import pickle

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import Optimizer
from mpi_opt_amd.search import make_parser
from oracle import gp_ei as O
from tests import committee_ref as R

LD = np.longdouble
MPO_EINVAL, MPO_ENOTSUP = 1, 3
PAD = {1: 4, 2: 4, 4: 4, 8: 8, 10: 12}
FIXTURES = [(40, 2, 3), (200, 10, 5), (97, 4, 2)]


def committee(n, d, E, seed=3, noise=0.02):
    X, y = O.synthetic_problem(n, d, seed=seed)
    c = R.Committee(X, y, 1.7, np.linspace(0.4, 1.3, d), noise, E=E)
    # the reference's experts are the optimizer's: the same rule at expert_size = ceil(n / E)
    parts = OPT.committee_partition(n, -(-n // E))
    assert len(parts) == E and all(np.array_equal(p, q) for p, q in zip(parts, c.parts))
    return c


# -- the reference against itself -------------------------------------------------------------
@pytest.mark.parametrize("n,d,E", FIXTURES)
def test_reference_p_at_least_one_and_precisions_agree(n, d, E):
    c = committee(n, d, E)
    C = O.synthetic_candidates(50, d, seed=5)
    mu, sd, P = c.posterior(C, "exact")
    mu64, sd64, P64 = c.posterior(C, "fp64")
    assert np.all(P.v >= 1) and np.all(P64.v >= 1)
    assert np.all(sd.v <= c.y_std * np.sqrt(LD(c.amp)))          # never less certain than the prior
    # the two restatements: fp64's own rounding, relative to the summand scales
    assert np.max(np.abs(np.asarray(mu.v - mu64.v, dtype=float)) / mu.s) < 1e-12
    assert np.max(np.abs(np.asarray(sd.v - sd64.v, dtype=float)) / sd.s) < 1e-12
    assert np.all(mu.s >= np.abs(np.asarray(mu.v, dtype=float))) and np.all(sd.s >= np.asarray(sd.v, dtype=float))


def test_reference_returns_the_prior_far_from_all_data():
    c = committee(97, 4, 2)
    mu, sd, P = c.posterior(np.full((3, 4), 60.0), "exact")
    assert np.all(P.v == 1)
    assert np.all(mu.v == LD(c.y_mean))
    assert np.max(np.abs(sd.v - LD(c.y_std) * np.sqrt(LD(c.amp)))) < 1e-18 * c.y_std
    r = c.value_grad(np.full(4, 60.0), 0.0, "LCB")
    assert np.all(r["mu_g"].v == 0) and np.all(r["sd_g"].v == 0)   # r_e = 1 is clamped: zero derivative


@pytest.mark.parametrize("n,d,E", FIXTURES)
def test_reference_gradient_matches_an_80_bit_central_difference(n, d, E):
    """Richardson-extrapolated central differences of the 80-bit values (steps h and h / 2,
    h = 2^-10: truncation O(h^4), rounding ~1e-19 / h) against the analytic gradient of the
    committee's mean, std and LCB.  Bar: 1e-8 of the gradient's summand scale."""
    c = committee(n, d, E)
    C = O.synthetic_candidates(4, d, seed=7)
    h = 2.0 ** -10

    def f(x):
        r = c.value_grad(x, 0.0, "LCB")
        return np.array([r["mu"].v, r["sd"].v, r["f"].v])

    def cd(x, j, step):
        xp, xm = x.copy(), x.copy()
        xp[j] += step
        xm[j] -= step
        return (f(xp) - f(xm)) / LD(xp[j] - xm[j])

    for x in C:
        r = c.value_grad(x, 0.0, "LCB")
        for j in range(d):
            num = (4 * cd(x, j, h / 2) - cd(x, j, h)) / 3
            for got, key in zip(num, ("mu_g", "sd_g", "g")):
                assert abs(float(got - r[key].v[j])) <= 1e-8 * r[key].s[j], (key, j)


def test_reference_ei_pi_gradients_match_central_differences():
    """EI and PI where they are not vanishing (y_opt above the data's mean)."""
    c = committee(200, 10, 5)
    x = O.synthetic_candidates(1, 10, seed=11)[0]
    y_opt = c.y_mean
    h = 2.0 ** -12
    for acq in ("EI", "PI"):
        r = c.value_grad(x, y_opt, acq)
        for j in range(10):
            def cd(step):
                xp, xm = x.copy(), x.copy()
                xp[j] += step
                xm[j] -= step
                return (c.value_grad(xp, y_opt, acq)["f"].v - c.value_grad(xm, y_opt, acq)["f"].v) / LD(xp[j] - xm[j])
            num = (4 * cd(h / 2) - cd(h)) / 3
            # scipy's cdf / pdf are fp64: their rounding (1e-16 |f|) over the step bounds the check
            assert abs(float(num - r["g"].v[j])) <= 1e-8 * r["g"].s[j] + 1e-15 * abs(float(r["f"].v)) / h, (acq, j)


# -- the partition rule -----------------------------------------------------------------------
@pytest.mark.parametrize("n,s", [(17, 16), (33, 16), (40, 16), (2049, 512), (4096, 512), (513, 512), (65536, 2048)])
def test_partition_rule(n, s):
    parts = OPT.committee_partition(n, s)
    E = -(-n // s)
    assert len(parts) == E == len(R.partition(n, s))
    sizes = [len(p) for p in parts]
    assert max(sizes) - min(sizes) <= 1 and max(sizes) <= s and sum(sizes) == n
    for e, p in enumerate(parts):
        assert np.array_equal(p % E, np.full(len(p), e)) and np.all(np.diff(p) == E)
        assert np.array_equal(p, R.partition(n, s)[e])


# -- ABI refusals on null-device structs ------------------------------------------------------
def expert(n=16, d=4, amp=1.5, y_mean=0.25, y_std=2.0, dp=None, np16=None, ptrs=True):
    m = _lib.MpoGpModel(n=n, d=d, dp=PAD[d] if dp is None else dp, np16=(n + 15) // 16 * 16 if np16 is None else np16,
                        amp=amp, y_mean=y_mean, y_std=y_std)
    if ptrs:
        for f in ("xs", "ls", "alpha", "W"):
            setattr(m, f, 4096)          # never dereferenced: every refusal is made on the host
    return m


def array(*models):
    arr = (_lib.MpoGpModel * len(models))()
    for i, m in enumerate(models):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(m), ctypes.sizeof(_lib.MpoGpModel))
    return arr


def entry_points(arr, E, m=100, k=1, ws_bytes=1 << 30):
    """Every committee entry point on the same host array: [(name, return code, message)]."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    calls = [
        ("mpo_gp_committee_check", lambda: L.mpo_gp_committee_check(arr, E, None)),
        ("mpo_gp_committee_score", lambda: L.mpo_gp_committee_score(arr, E, p, m, 0.0, 0.01, 1.96, 1, p, p, p, k, p, p,
                                                                    p, ws_bytes, None)),
        ("mpo_gp_committee_grad", lambda: L.mpo_gp_committee_grad(arr, E, p, 1, p, 0.0, 0.01, 1.96, p, p, None)),
        ("mpo_gp_committee_grad_host", lambda: L.mpo_gp_committee_grad_host(arr, E, p, 1, p, 0.0, 0.01, 1.96, p, p,
                                                                            None)),
    ]
    out = []
    for name, call in calls:
        rc = call()
        out.append((name, rc, L.mpo_last_error().decode()))
    return out


@pytest.mark.parametrize("E", [0, -1, 33])
def test_refuses_expert_counts_outside_1_to_32(E):
    arr = array(*[expert() for _ in range(33)])
    for name, rc, msg in entry_points(arr, E):
        assert rc == MPO_EINVAL and name in msg and f"E={E} outside [1, 32]" in msg, (name, rc, msg)
    assert _lib.lib().mpo_gp_committee_ws_bytes(arr, E, 100, 1) == 0
    assert _lib.lib().mpo_gp_committee_grad_path(arr, E) == -MPO_EINVAL
    assert _lib.MPO_COMMITTEE_MAX == 32


@pytest.mark.parametrize("other,what", [
    (dict(d=8), "differs in shape"), (dict(dp=8), "differs in shape"), (dict(amp=1.5000000000000002), "differs in amp"),
    (dict(y_mean=0.5), "differs in the target normalisation"), (dict(y_std=2.5), "differs in the target normalisation")])
def test_refuses_experts_that_differ(other, what):
    arr = array(expert(), expert(), expert(**other))
    for name, rc, msg in entry_points(arr, 3):
        assert rc == MPO_EINVAL and name in msg and "expert 2" in msg and what in msg, (name, rc, msg)
    assert _lib.lib().mpo_gp_committee_ws_bytes(arr, 3, 100, 1) == 0
    assert _lib.lib().mpo_gp_committee_ws_bytes(arr, 2, 100, 1) > 0       # the first two agree


def test_refuses_an_expert_past_2048_rows():
    arr = array(expert(), expert(n=2049))
    for name, rc, msg in entry_points(arr, 2):
        assert rc == MPO_ENOTSUP and name in msg and "expert 1" in msg and "n=2049" in msg and "2048" in msg, (name, msg)
    assert _lib.lib().mpo_gp_committee_ws_bytes(arr, 2, 100, 1) == 0
    assert _lib.lib().mpo_gp_committee_ws_bytes(array(expert(), expert(n=2048)), 2, 100, 1) > 0


@pytest.mark.parametrize("bad", [dict(ptrs=False), dict(n=0), dict(np16=17), dict(np16=48), dict(dp=2),
                                 dict(y_std=0.0), dict(amp=0.0)])
def test_refuses_a_malformed_expert(bad):
    arr = array(expert(**bad), expert())
    for name, rc, msg in entry_points(arr, 2):
        assert rc == MPO_EINVAL and name in msg and "expert 0: null or unprepared model" in msg, (name, rc, msg)
    for name, rc, msg in entry_points(None, 2):
        assert rc == MPO_EINVAL and "null models" in msg


def test_score_refuses_bad_arguments():
    L = _lib.lib()
    arr = array(expert(), expert(n=15))
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    need = L.mpo_gp_committee_ws_bytes(arr, 2, 100, 1)
    assert need > 0

    def score(m=100, flags=1, k=1, mu=p, vals=p, tk=p, ws=p, ws_bytes=need, cand=p):
        rc = L.mpo_gp_committee_score(arr, 2, cand, m, 0.0, 0.01, 1.96, flags, mu, mu, vals, k, tk, tk, ws, ws_bytes, None)
        return rc, L.mpo_last_error().decode()

    assert score(k=_lib.MPO_TOPK_MAX + 1) == (MPO_EINVAL, "mpo_gp_committee_score: k=9 outside [0,8]")
    assert L.mpo_gp_committee_ws_bytes(arr, 2, 100, _lib.MPO_TOPK_MAX + 1) == 0
    rc, msg = score(ws_bytes=need - 1)
    assert rc == MPO_EINVAL and "workspace too small" in msg and str(need) in msg
    rc, msg = score(ws=None)
    assert rc == MPO_EINVAL and "workspace too small" in msg
    assert score(m=0) == (MPO_EINVAL, "mpo_gp_committee_score: m must be > 0")
    assert score(flags=8)[0] == MPO_EINVAL and "bad flags 8" in score(flags=8)[1]
    assert score(flags=0)[0] == MPO_EINVAL
    assert score(tk=None) == (MPO_EINVAL, "mpo_gp_committee_score: topk outputs required for k>0")
    assert score(k=0, mu=None, vals=None) == (MPO_EINVAL, "mpo_gp_committee_score: nothing to compute")
    assert score(cand=None) == (MPO_EINVAL, "mpo_gp_committee_score: null candidates")
    rc = L.mpo_gp_committee_grad(arr, 2, p, 0, p, 0.0, 0.01, 1.96, p, p, None)
    assert rc == MPO_EINVAL and "batch=0 outside [1, 65535]" in L.mpo_last_error().decode()
    rc = L.mpo_gp_committee_grad(arr, 2, None, 1, p, 0.0, 0.01, 1.96, p, p, None)
    assert rc == MPO_EINVAL and "null pointer" in L.mpo_last_error().decode()
    opts = _lib.MpoLbfgsbOptions(1e-9, 1e-5, 20, 15000, 10, 20)
    rc = L.mpo_gp_polish_committee_host(arr, 33, p, p, 1, p, ctypes.byref(opts), 0.0, 0.01, 1.96, p, p, p, p, p, p, p,
                                        p, None)
    assert rc == MPO_EINVAL and "E=33 outside [1, 32]" in L.mpo_last_error().decode()


@pytest.mark.parametrize("m", [10_000, 1_000_000])
def test_workspace_does_not_grow_with_the_number_of_experts(m):
    """E from 2 to 32 at a fixed largest expert: less than one [m] row more (here: nothing), and
    at 10^6 candidates and 32 experts tens of MB."""
    L = _lib.lib()
    ws = {E: L.mpo_gp_committee_ws_bytes(array(*[expert(n=512, d=10) for _ in range(E)]), E, m, 5) for E in (1, 2, 32)}
    assert ws[2] > 0 and ws[32] - ws[2] < 8 * m
    one = L.mpo_gp_score_ws_bytes(ctypes.byref(expert(n=512, d=10)), m, 0)
    assert ws[32] <= one + 4 * 8 * m + (1 << 20)                 # the expert's own workspace + four rows + top-k lists
    if m == 1_000_000:
        assert ws[32] < 64 << 20
    # the largest expert decides, wherever it stands
    mixed = array(expert(n=100, d=10), expert(n=2048, d=10), expert(n=100, d=10))
    grown = L.mpo_gp_score_ws_bytes(ctypes.byref(expert(n=2048, d=10)), m, 0) - one
    assert abs(L.mpo_gp_committee_ws_bytes(mixed, 3, m, 5) - ws[2] - grown) < 256      # the carver's alignment


# -- the refit objective: a sum over the experts ------------------------------------------------
class StubLML:
    """An expert's ``evaluate`` with known values: lml = c sum(theta), grad = c, info as given."""

    def __init__(self, c, bad_rows=()):
        self.c, self.bad_rows, self.calls = c, tuple(bad_rows), 0

    def evaluate(self, thetas):
        self.calls += 1
        B, k = thetas.shape
        info = np.zeros(B, dtype=np.int32)
        lml, grad = self.c * thetas.sum(1), np.full((B, k), float(self.c))
        for r in self.bad_rows:
            info[r], lml[r], grad[r] = 7 + r, -np.inf, 0.0
        return lml, grad, info


def test_refit_objective_sums_every_expert_and_reports_a_failed_one():
    experts = [StubLML(1.0), StubLML(10.0, bad_rows=(1,)), StubLML(100.0)]
    th = np.array([[0.5, -1.0, 2.0], [1.0, 1.0, 1.0], [0.0, 0.25, -0.25]])
    lml, grad, info = OPT.summed_lml_objective(experts)(th)
    assert [e.calls for e in experts] == [1, 1, 1]
    assert np.array_equal(lml[[0, 2]], ((1.0 * th.sum(1) + 10.0 * th.sum(1)) + 100.0 * th.sum(1))[[0, 2]])
    assert np.array_equal(grad[[0, 2]], np.full((2, 3), 111.0))
    assert list(info) == [0, 8, 0] and lml[1] == -np.inf and np.all(grad[1] == 0.0)
    # the first failed expert's info is the one reported; a 1-D theta is one row
    lml, grad, info = OPT.summed_lml_objective([StubLML(1.0, (0,)), StubLML(2.0, (0,))])(np.array([1.0, 2.0]))
    assert list(info) == [7] and lml[0] == -np.inf and grad.shape == (1, 2) and np.all(grad == 0.0)
    lml, grad, info = OPT.summed_lml_objective([StubLML(3.0)])(np.array([[1.0, 2.0]]))
    assert lml[0] == 9.0 and np.all(grad == 3.0) and info[0] == 0


def test_polish_entry_point_runs_the_shared_host_check():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    opts = _lib.MpoLbfgsbOptions(1e-9, 1e-5, 20, 15000, 10, 20)

    def polish(arr, E):
        rc = L.mpo_gp_polish_committee_host(arr, E, p, p, 1, p, ctypes.byref(opts), 0.0, 0.01, 1.96, p, p, p, p, p, p,
                                            p, p, None)
        return rc, L.mpo_last_error().decode()

    assert polish(None, 2) == (MPO_EINVAL, "mpo_gp_polish_committee_host: null models")
    assert polish(array(expert(), expert()), 33) == (MPO_EINVAL, "mpo_gp_polish_committee_host: E=33 outside [1, 32]")
    rc, msg = polish(array(expert(ptrs=False), expert()), 2)
    assert rc == MPO_EINVAL and msg == "mpo_gp_polish_committee_host: expert 0: null or unprepared model"
    rc, msg = polish(array(expert(), expert(amp=2.0)), 2)
    assert rc == MPO_EINVAL and "expert 1 differs in amp" in msg
    rc, msg = polish(array(expert(), expert(n=2049)), 2)
    assert rc == MPO_ENOTSUP and "expert 1: n=2049" in msg


# -- the optimizer's keywords -----------------------------------------------------------------
SPACE = [(0.0, 1.0), (0.0, 1.0)]


def test_constructor_refusals():
    with pytest.raises(ValueError, match="surrogate 'rbcm': one of"):
        Optimizer(SPACE, surrogate="rbcm")
    for bad in (15, 2049, 512.0, "512", True, None):
        with pytest.raises(ValueError, match=r"expert_size .*: an int in \[16, 2048\]"):
            Optimizer(SPACE, expert_size=bad)
    with pytest.raises(ValueError, match='surrogate="committee" with lie_refit="never" is not supported: '):
        Optimizer(SPACE, surrogate="committee", lie_refit="never")
    with pytest.raises(ValueError, match='surrogate="committee" with the "thompson" strategy is not supported: '):
        Optimizer(SPACE, surrogate="committee", batch_strategy="thompson")
    for acq in ("EIps", "PIps"):
        with pytest.raises(ValueError, match=f'surrogate="committee" with acq_func \'{acq}\' is not supported: '):
            Optimizer(SPACE, surrogate="committee", acq_func=acq)
    with pytest.raises(ValueError, match='surrogate="committee" with the "thompson" strategy'):
        Optimizer(SPACE, surrogate="committee").ask(2, strategy="thompson")
    opt = Optimizer(SPACE, surrogate="committee", expert_size=16, random_state=1)
    assert (opt.surrogate, opt.expert_size) == ("committee", 16)
    assert (Optimizer(SPACE).surrogate, Optimizer(SPACE).expert_size) == ("exact", 512)
    # a copy and a chain job carry both
    cfg = opt._config()
    assert (cfg["surrogate"], cfg["expert_size"]) == ("committee", 16)
    cp = opt.copy(random_state=3)
    assert (cp.surrogate, cp.expert_size) == ("committee", 16)


def told(n, **kw):
    opt = Optimizer(SPACE, acq_func="EI", random_state=0, n_initial_points=100000, **kw)
    pts = [[i / float(n), 0.5] for i in range(n)]
    opt.tell(pts, [p[0] for p in pts])              # still inside the initial points: no GP
    opt._n_initial_points = 0
    return opt


def test_size_limits_before_any_device_work():
    """No GPU here: the ValueError must come before the refit touches a device."""
    opt = told(2040)                                # the default surrogate still stops at 2048
    with pytest.raises(ValueError, match=r"2048.*lies"):
        opt.tell([[0.1, 0.2]] * 9, [0.0] * 9)
    assert len(opt.yi) == 2040
    opt = told(32 * 16 - 3, surrogate="committee", expert_size=16)
    with pytest.raises(ValueError, match=r"32 experts of expert_size = 16 observations \(512\), got n = 513"):
        opt.tell([[0.1, 0.2]] * 4, [0.0] * 4)
    assert len(opt.yi) == 32 * 16 - 3
    with pytest.raises(ValueError, match=r"32 experts of expert_size = 16 .*509 told points \+ 4 constant-liar lies"):
        opt.ask(4)


def test_pickle_round_trip_and_old_checkpoints():
    opt = told(40, surrogate="committee", expert_size=16)
    back = pickle.loads(pickle.dumps(opt))
    assert (back.surrogate, back.expert_size, len(back.yi)) == ("committee", 16, 40)
    assert back._config()["surrogate"] == "committee"
    # a checkpoint written before the keywords existed resumes with the defaults
    old = Optimizer(SPACE, random_state=0)
    state = old.__getstate__()
    del state["surrogate"], state["expert_size"]
    fresh = Optimizer.__new__(Optimizer)
    fresh.__setstate__(state)
    assert (fresh.surrogate, fresh.expert_size) == ("exact", 512)
    assert fresh._config()["expert_size"] == 512 and fresh._committee_size is None


def test_committee_model_pickles_without_device_state_and_refuses_joint_calls():
    X, y = O.synthetic_problem(40, 2, seed=3)
    m = OPT.CommitteeModel(X, y, 1.7, [0.5, 0.9], 0.02, 16)
    assert len(m.estimators_) == 3 and [len(e.y) for e in m.estimators_] == [14, 13, 13]
    assert all(e.norm == m.norm for e in m.estimators_) and m.norm == (float(np.mean(y)), float(np.std(y)))
    assert np.array_equal(m.estimators_[1].y, y[1::3]) and np.array_equal(m.estimators_[1].Xt, X[1::3])
    assert (m.amp, m.noise, list(m.length_scale)) == (1.7, 0.02, [0.5, 0.9]) and np.array_equal(m.y, y)
    back = pickle.loads(pickle.dumps(m))
    assert back._com is None and all(e._dev is None for e in back.estimators_) and back.norm == m.norm
    for call in (lambda: m.predict(X[:2], return_cov=True), lambda: m.sample_y(X[:2]), lambda: m.sample_paths()):
        with pytest.raises(ValueError, match='"committee" surrogate'):
            call()
    with pytest.raises(ValueError, match="n > expert_size"):
        OPT.CommitteeModel(X[:16], y[:16], 1.7, [0.5, 0.9], 0.02, 16)
    from mpi_opt_amd import analysis

    opt = told(40, surrogate="committee", expert_size=16)
    opt.models.append(m)
    for call in (lambda: analysis.objective_report(opt), lambda: analysis.expected_minimum(opt),
                 lambda: analysis.partial_dependence(opt.space, m, 0)):
        with pytest.raises(ValueError, match='do not take the "committee" surrogate'):
            call()


def test_cli_flags():
    p = make_parser()
    a = p.parse_args([])
    assert (a.surrogate, a.expert_size) == ("exact", 512)
    a = p.parse_args(["--surrogate", "committee", "--expert-size", "16"])
    assert (a.surrogate, a.expert_size) == ("committee", 16)
    with pytest.raises(SystemExit):
        p.parse_args(["--surrogate", "sparse"])
    flag = next(x for x in p._actions if "--surrogate" in x.option_strings)
    assert "NOT the reference" in flag.help and "search quality" in flag.help
