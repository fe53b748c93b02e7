"""``Optimizer(candidates="device")`` on the GPU: a proposal draws one seed and scores
candidates written by ``mpo_space_sample``.  Not skopt's stream, so there is no oracle
trace; the checks are that a device-mode proposal is exactly what the same candidate
bits give when they are fed through the host path (numpy array, host-to-device copy,
the same scoring kernel: top-k, polished points and picks equal, nothing skipped), that
the asking RandomState advances by the one seed draw, and that the default mode is
untouched.  The told set is that of tests/test_lie_refit_gpu.py."""
import pickle

import numpy as np
import pytest
import torch

from mpi_opt_amd.blocks import ShardedScorer, _device_topk
from mpi_opt_amd.candidates import sample_transformed
from mpi_opt_amd.optimizer import Optimizer
from mpi_opt_amd.space import Integer, Real, Space
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

ACQS = ("EI", "LCB", "PI")
SEED = 4
N_POINTS = 2000
INT32_MAX = np.iinfo(np.int32).max


def space():
    return [Real(-2.0, 2.0), Real(1e-3, 1.0, prior="log-uniform"), Integer(3, 9)]


def objective(p):
    return float((p[0] - 0.5) ** 2 + (np.log10(p[1]) + 1.5) ** 2 + 0.1 * (p[2] - 6) ** 2)


def told_optimizer(n_told=12, trace=True, n_points=N_POINTS, **kw):
    opt = Optimizer(space(), random_state=SEED, n_initial_points=10, acq_optimizer_kwargs={"n_points": n_points},
                    **kw)
    pts = opt.space.rvs(n_samples=n_told, random_state=np.random.RandomState(SEED + 1))
    if trace:
        opt.trace = []
    opt.tell(pts, [objective(p) for p in pts])
    return opt


def reference_candidates(rec, n_points=N_POINTS):
    return P.sample_transformed(space(), n_points, rec["cand_seed"])


def test_device_mode_proposes_what_its_candidates_give_through_the_host_path(monkeypatch):
    models = []
    propose = Optimizer._propose

    def recording(self, est, *a, **kw):
        models.append(est)
        return propose(self, est, *a, **kw)

    monkeypatch.setattr(Optimizer, "_propose", recording)
    opt = told_optimizer(candidates="device")
    Xa = opt.ask(4)
    ta = opt.trace + opt.batch_trace                  # the tell, the copy's own fit, one record per lie
    assert len(ta) == len(models) == 6
    monkeypatch.setattr(Optimizer, "_propose", propose)

    # (1) every record: the reference rows of its seed, as a numpy array on the record's model
    for rec, est in zip(ta, models):
        assert 0 <= rec["cand_seed"] < INT32_MAX
        Xr = reference_candidates(rec)
        top = _device_topk(est, Xr, float(np.min(est.y)), ACQS, 0.01, 1.96, 5)
        for acq in ACQS:
            np.testing.assert_array_equal(rec["top"][acq], top[acq][1], err_msg=acq)

    # (2) the whole run again in host mode, its candidate draw replaced by the reference of
    # the same one seed draw: the host path end to end on equal candidate bits
    def host_fed(self, n_samples=1, random_state=None):
        return P.sample_transformed(self.dimensions, n_samples, int(random_state.randint(0, INT32_MAX)))

    monkeypatch.setattr(Space, "rvs_transformed", host_fed)
    ref = told_optimizer(candidates="host")
    Xb = ref.ask(4)
    tb = ref.trace + ref.batch_trace
    assert len(tb) == 6 and all("cand_seed" not in rec for rec in tb)      # host records keep their keys
    for ra, rb in zip(ta, tb):
        assert ra["theta"][0] == rb["theta"][0] and np.array_equal(ra["theta"][1], rb["theta"][1])
        for acq in ACQS:
            np.testing.assert_array_equal(ra["top"][acq], rb["top"][acq])
            np.testing.assert_array_equal(ra["polished"][acq][0], rb["polished"][acq][0])
            np.testing.assert_array_equal(ra["polished"][acq][1], rb["polished"][acq][1])
        assert ra["pick"] == rb["pick"]
    assert [list(p) for p in Xa] == [list(p) for p in Xb]
    assert opt.rng.randint(0, 1 << 30) == ref.rng.randint(0, 1 << 30)


def test_large_candidate_set_scores_as_the_host_fed_reference():
    """200 003 candidates: not a multiple of the scoring kernel's 16-candidate tile and
    past one resident grid of it.  For the sampler this is a single pass (2 pairs x 200 003
    rows are fewer items than its grid); tests/test_candidates_gpu.py has its multi-pass cases."""
    n = 200_003
    est = told_optimizer(n_told=16, trace=False).models[-1]
    Xd = sample_transformed(Space(space()), n, 99, "cuda:0")
    Xh = P.sample_transformed(space(), n, 99)
    assert np.array_equal(Xd.cpu().numpy(), Xh)
    y_opt = float(np.min(est.y))
    td = _device_topk(est, Xd, y_opt, ACQS, 0.01, 1.96, 5)
    th = _device_topk(est, Xh, y_opt, ACQS, 0.01, 1.96, 5)
    for acq in ACQS:
        assert len(td[acq][1]) == 5
        np.testing.assert_array_equal(td[acq][1], th[acq][1])
        np.testing.assert_array_equal(td[acq][0], th[acq][0])


def test_equal_optimizers_give_equal_batches():
    a = told_optimizer(trace=False, candidates="device").ask(4)
    b = told_optimizer(trace=False, candidates="device").ask(4)
    assert [list(p) for p in a] == [list(p) for p in b]
    assert len({tuple(p) for p in a}) == 4
    for p in a:
        assert -2.0 <= p[0] <= 2.0 and 1e-3 <= p[1] <= 1.0 and p[2] in range(3, 10) and float(p[2]) == int(p[2])


def test_threaded_chains_give_the_inline_points():
    """Chain workers sample and score on their own streams: same batch as the inline ask."""
    from mpi_opt_amd.chains import ThreadChainExecutor

    inline = told_optimizer(trace=False, candidates="device").ask(4)
    ex = ThreadChainExecutor("cuda:0", workers=2)
    try:
        opt = told_optimizer(trace=False, candidates="device", chain_executor=ex)
        threaded = [list(p) for p in opt.ask(4)]
    finally:
        ex.close()
    assert threaded == [list(p) for p in inline]


def test_a_proposal_advances_the_rng_by_the_one_seed_draw():
    # a single acquisition: no gp_hedge multinomial draw, the seed is the proposal's only one
    opt = told_optimizer(candidates="device", acq_func="EI")
    for _ in range(2):
        probe = pickle.loads(pickle.dumps(opt.rng))
        x = opt.ask()
        opt.tell(x, objective(x))
        assert opt.trace[-1]["cand_seed"] == probe.randint(0, INT32_MAX)
        assert opt.rng.randint(0, 1 << 30) == probe.randint(0, 1 << 30)
    # an ask(n) draws the copy's seed and nothing else: the candidate seeds come from the copy
    probe = pickle.loads(pickle.dumps(opt.rng))
    probe.randint(0, INT32_MAX)
    assert len(opt.ask(2)) == 2
    assert opt.rng.randint(0, 1 << 30) == probe.randint(0, 1 << 30)


def test_explicit_host_mode_is_the_default():
    a, b = told_optimizer(), told_optimizer(candidates="host")
    for _ in range(2):
        xa, xb = a.ask(), b.ask()
        assert list(xa) == list(xb)
        a.tell(xa, objective(xa))
        b.tell(xb, objective(xb))
    assert [list(p) for p in a.ask(3)] == [list(p) for p in b.ask(3)]
    assert all("cand_seed" not in rec for rec in a.trace + b.trace + b.batch_trace)
    sa, sb = a.rng.get_state(), b.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_sampling_mode_returns_a_candidate_row():
    opt = told_optimizer(candidates="device", acq_optimizer="sampling")
    rec = opt.trace[-1]
    Xr = reference_candidates(rec)
    for acq, nx in zip(ACQS, opt.next_xs_):
        assert np.array_equal(nx, Xr[rec["top"][acq][0]])
    x = opt.ask()
    assert opt.space.inverse_transform(opt.next_xs_[rec["pick"]].reshape(1, -1))[0] == x
    assert x[2] in range(3, 10)


def test_sharded_scorer_scores_a_device_tensor_locally():
    class NoOtherRanks:                               # a second rank that must never be asked
        world = 2

        def score(self, req):
            raise AssertionError("a device tensor was sent to the ranks")

    scorer = ShardedScorer(NoOtherRanks(), min_shard=1)
    opt = told_optimizer(candidates="device", scorer=scorer)
    assert (scorer.local_requests, scorer.sharded_requests) == (1, 0)
    rec, est = opt.trace[-1], opt.models[-1]
    Xd = sample_transformed(opt.space, N_POINTS, rec["cand_seed"], "cuda:0")
    assert isinstance(Xd, torch.Tensor) and Xd.is_cuda
    top = scorer(est, Xd, float(np.min(est.y)), ACQS, 0.01, 1.96, 5)
    assert (scorer.local_requests, scorer.sharded_requests) == (2, 0)
    for acq in ACQS:
        np.testing.assert_array_equal(top[acq], rec["top"][acq])
    with pytest.raises(AssertionError, match="sent to the ranks"):      # a host array of that size is still split
        scorer(est, Xd.cpu().numpy(), float(np.min(est.y)), ACQS, 0.01, 1.96, 5)
