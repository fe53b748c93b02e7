"""Retiring early-stopped members from the population engines
(``mpo_pop_set_active`` / ``mpo_dn_set_active``): a retired member is frozen bit
for bit, an active member's bits are those of the same steps with nobody retired,
and the fold loop / TrialEvaluator give the same answers with and without it.
Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (F, k, p, dense): every NT bucket, k <= 4 (dgf list) and k > 4 (dgrad list), members with
# >= 3 weight-gradient m-groups; batch 10 is not a multiple of the 4-sample slab groups
MEMBERS = [(10, 2, 2, 50), (50, 10, 10, 200), (33, 5, 3, 77), (17, 3, 7, 120), (50, 5, 2, 200), (16, 7, 4, 64)]
BATCH, N_SAMPLES, STEPS = 10, 60, 4
RETIRED = [0, 2, 5]
ACTIVE = [1, 3, 4]
NT1 = [0, 5]        # F <= 16
SMALL_K = [0, 3]    # k <= 4


def mask(n, retired):
    m = np.ones(n, dtype=bool)
    m[list(retired)] = False
    return m


def mnist_engine():
    from mpi_opt_amd.population import PopulationEngine, TrialSpec, glorot_uniform_init

    specs = [TrialSpec(F, k, p, d, 1e-3 * (1 + i), 0.25, seed=500 + i) for i, (F, k, p, d) in enumerate(MEMBERS)]
    init = [glorot_uniform_init(s, 11 + i) for i, s in enumerate(specs)]
    return PopulationEngine(specs, batch=BATCH, init=init)


def mnist_slices(eng, t):
    """Member slices of a parameter-arena tensor."""
    return [t[o[0]:o[8]] for o in eng.layout]


@pytest.fixture(scope="module")
def mnist_ref():
    """Engine B: STEPS steps with nobody retired; (params, m, v, loss) after each step,
    and the validation sums of one batch after the last."""
    rng = np.random.RandomState(3)
    x = torch.from_numpy(rng.uniform(size=(N_SAMPLES, 784)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, 10, size=N_SAMPLES).astype(np.int32)).cuda()
    order = torch.from_numpy(np.stack([rng.permutation(N_SAMPLES).astype(np.int32) for _ in MEMBERS])).cuda()
    B = mnist_engine()
    snaps = []
    for s in range(STEPS):
        B.train_step(x, y, order, s * BATCH, step=s)
        snaps.append(tuple(t.clone() for t in (B.params, B.adam_m, B.adam_v, B.loss)))
    B.eval_reset()
    B.eval_step(x, y, order, 4 * BATCH)
    val = (B.val_loss_sum.clone(), B.val_correct.clone())
    return dict(x=x, y=y, order=order, snaps=snaps, val=val, work=B.step_work())


def assert_members_equal(eng, got, want, members, what):
    g, w = mnist_slices(eng, got), mnist_slices(eng, want)
    for i in members:
        assert torch.equal(g[i], w[i]), f"member {i}: {what}"


def test_mnist_retired_members_freeze_and_active_members_keep_their_bits(mnist_ref):
    r = mnist_ref
    A = mnist_engine()
    assert A.step_work() == r["work"] and A.active.all()
    for s in range(2):
        A.train_step(r["x"], r["y"], r["order"], s * BATCH, step=s)
    A.set_active(mask(len(MEMBERS), RETIRED))
    assert A.active.tolist() == mask(len(MEMBERS), RETIRED).tolist()
    assert 0 < A.step_work()[0] < r["work"][0]
    for s in range(2, 4):
        A.train_step(r["x"], r["y"], r["order"], s * BATCH, step=s)
    for j, name in enumerate(("params", "adam m", "adam v")):
        got = (A.params, A.adam_m, A.adam_v)[j]
        assert_members_equal(A, got, r["snaps"][3][j], ACTIVE, f"{name} differs from the unmasked run after step 4")
        assert_members_equal(A, got, r["snaps"][1][j], RETIRED, f"{name} moved after the member was retired")
    assert torch.equal(A.loss[ACTIVE], r["snaps"][3][3][ACTIVE])
    assert torch.equal(A.loss[RETIRED], r["snaps"][1][3][RETIRED])
    A.eval_reset()
    A.eval_step(r["x"], r["y"], r["order"], 4 * BATCH)
    assert torch.equal(A.val_loss_sum[ACTIVE], r["val"][0][ACTIVE])
    assert torch.equal(A.val_correct[ACTIVE], r["val"][1][ACTIVE])
    assert not A.val_loss_sum[RETIRED].any() and not A.val_correct[RETIRED].any()
    assert A.val_loss_sum[ACTIVE].all()          # the comparison above is not one of zeros


def test_mnist_masks_that_empty_launches(mnist_ref):
    r = mnist_ref
    A = mnist_engine()
    for s, retired in enumerate((NT1, SMALL_K)):
        A.set_active(mask(len(MEMBERS), retired))
        before = A.params.clone()
        A.train_step(r["x"], r["y"], r["order"], s * BATCH, step=s)
        A.eval_step(r["x"], r["y"], r["order"], 4 * BATCH)
        torch.cuda.synchronize()
        assert_members_equal(A, A.params, before, retired, "a retired member's parameters moved")
        moved = [not torch.equal(a, b) for a, b in zip(mnist_slices(A, A.params), mnist_slices(A, before))]
        assert moved == mask(len(MEMBERS), retired).tolist()
    A.set_active(np.zeros(len(MEMBERS), dtype=bool))
    assert A.step_work() == (0, 0)
    before = tuple(t.clone() for t in (A.params, A.adam_m, A.adam_v, A.loss, A.val_loss_sum))
    A.train_step(r["x"], r["y"], r["order"], 2 * BATCH, step=2)
    A.eval_step(r["x"], r["y"], r["order"], 4 * BATCH)
    torch.cuda.synchronize()
    for a, b in zip((A.params, A.adam_m, A.adam_v, A.loss, A.val_loss_sum), before):
        assert torch.equal(a, b)


def test_mnist_reactivation(mnist_ref):
    r = mnist_ref
    A = mnist_engine()
    for s in range(2):
        A.train_step(r["x"], r["y"], r["order"], s * BATCH, step=s)
    A.set_active(mask(len(MEMBERS), RETIRED))
    A.train_step(r["x"], r["y"], r["order"], 2 * BATCH, step=2)
    A.set_active(np.ones(len(MEMBERS), dtype=bool))
    assert A.step_work() == r["work"]
    before = A.params.clone()
    A.train_step(r["x"], r["y"], r["order"], 3 * BATCH, step=3)
    assert_members_equal(A, A.params, r["snaps"][3][0], ACTIVE, "left the unmasked trajectory after re-activation")
    for i in RETIRED:
        assert not torch.equal(mnist_slices(A, A.params)[i], mnist_slices(A, before)[i]), f"member {i} did not step"


DN_CASES = [
    # scalar BN path (odd channel counts)
    dict(img=(8, 8, 3), depth=7, blocks=2, growth=5, nbf=7, B=4),
    # float4 BN, streamed 1x1 conv, BN backward reduce fused into the input-gradient conv
    dict(img=(16, 16, 3), depth=7, blocks=3, growth=12, nbf=16, B=8),
]


def dn_population(case):
    from mpi_opt_amd.densenet import DenseNetArch, DenseNetPopulation, he_uniform_init

    arch = DenseNetArch(img_dim=case["img"], nb_classes=10, depth=case["depth"], nb_dense_block=case["blocks"],
                        growth_rate=case["growth"], nb_filter=case["nbf"])
    init = [he_uniform_init(arch.layers(), 21 + i) for i in range(4)]
    return DenseNetPopulation(arch, [1e-3, 2e-3, 3e-3, 4e-3], batch=case["B"], init=init)


def dn_tensors(pop):
    return pop.params, pop.state, pop.adam_m, pop.adam_v


@pytest.mark.parametrize("case", DN_CASES, ids=["scalar-bn", "vec4-c1x1-fused"])
def test_densenet_retired_members_freeze_and_active_members_keep_their_bits(case):
    B = case["B"]
    n_samples = 5 * B
    rng = np.random.RandomState(9)
    x = torch.from_numpy(rng.rand(n_samples, *case["img"]).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, 10, n_samples).astype(np.int32)).cuda()
    order = torch.from_numpy(np.stack([rng.permutation(n_samples).astype(np.int32) for _ in range(4)])).cuda()
    ref = dn_population(case)
    snaps = {}
    for s in range(5):
        ref.train_step(x, y, order, s * B, step=s)
        snaps[s + 1] = tuple(t.clone() for t in dn_tensors(ref)) + (ref.loss.clone(),)
        if s == 3:
            ref.eval_reset()
            ref.eval_step(x, y, order, 0)
            val = (ref.val_loss_sum.clone(), ref.val_correct.clone())
    retired, active = [0, 2], [1, 3]        # the table of active members is not a prefix
    A = dn_population(case)
    work0 = A.step_work()
    for s in range(2):
        A.train_step(x, y, order, s * B, step=s)
    A.set_active(mask(4, retired))
    assert A.step_work()[0] < work0[0] and A.step_work()[1] == work0[1]
    for s in range(2, 4):
        A.train_step(x, y, order, s * B, step=s)
    for j, name in enumerate(("params", "state", "adam m", "adam v")):
        got = dn_tensors(A)[j]
        assert torch.equal(got[active], snaps[4][j][active]), f"active members' {name} differ from the unmasked run"
        assert torch.equal(got[retired], snaps[2][j][retired]), f"retired members' {name} moved"
    assert torch.equal(A.loss[active], snaps[4][4][active]) and torch.equal(A.loss[retired], snaps[2][4][retired])
    A.eval_reset()
    A.eval_step(x, y, order, 0)
    assert torch.equal(A.val_loss_sum[active], val[0][active]) and torch.equal(A.val_correct[active], val[1][active])
    assert not A.val_loss_sum[retired].any() and not A.val_correct[retired].any()
    assert A.val_loss_sum[active].all()
    assert A.penalty().cpu().numpy().all()       # the penalty still covers every member
    # all retired: a step launches nothing
    A.set_active(np.zeros(4, dtype=bool))
    assert A.step_work() == (0, 0)
    before = tuple(t.clone() for t in dn_tensors(A)) + (A.loss.clone(),)
    A.train_step(x, y, order, 4 * B, step=4)
    A.eval_step(x, y, order, 0)
    torch.cuda.synchronize()
    for a, b in zip(dn_tensors(A) + (A.loss,), before):
        assert torch.equal(a, b)
    # all active again: members 1 and 3 are back on the unmasked trajectory's step 5
    A.set_active(np.ones(4, dtype=bool))
    assert A.step_work() == work0
    A.train_step(x, y, order, 4 * B, step=4)
    for j in range(4):
        assert torch.equal(dn_tensors(A)[j][active], snaps[5][j][active])
    assert not torch.equal(A.params[retired], before[0][retired])


SEARCH_LR = 1e-3
SEARCH_PARAMS = [[10, 2, 2, 50, 0.1], [25, 4, 3, 80, 0.7], [50, 10, 10, 200, 0.2], [33, 5, 3, 77, 0.25],
                 [16, 7, 4, 64, 0.5]]


def test_search_path_gives_the_same_answers():
    """TrialEvaluator with and without retiring: identical FOMs and histories, and the
    retiring run skipped member-epochs.  Patience 1 over 3 epochs; the learning rate
    makes some members stop after epoch 2 while others run all 3 (asserted)."""
    from mpi_opt_amd.blocks import TrialEvaluator
    from mpi_opt_amd.models import BuilderFromFunction, mnist_space
    from mpi_opt_amd.models import test_mnist as mnist_fn
    from mpi_opt_amd.population import synthetic_mnist
    from mpi_opt_amd.stopping import StopRule

    x, y = synthetic_mnist(600, seed=3, labels="learnable")
    out = {}
    for retire in (False, True):
        ev = TrialEvaluator(BuilderFromFunction(mnist_fn, mnist_space()), x, y, n_fold=2, epochs=3, batch=50, lr=SEARCH_LR,
                            stopping=StopRule.from_args("1"), retire_stopped=retire)
        units = ev.units(SEARCH_PARAMS)
        res = ev.train_units(units)
        out[retire] = (ev.foms(SEARCH_PARAMS, res), res, ev.member_epochs_skipped)
    lengths = [len(h["val_loss"]) for h in out[False][1].values()]
    print("history lengths without retiring:", lengths)
    assert min(lengths) < 3, "no member stopped before the last epoch: the comparison would be vacuous"
    assert out[True][0] == out[False][0]
    assert out[True][1] == out[False][1]
    assert out[False][2] == 0 and out[True][2] > 0
    assert all(np.isfinite(v) for h in out[True][1].values() for v in h["val_loss"])



class _ScriptedRule:
    """A target rule whose members reach it on script: member i stops after epoch
    ``stop_after[i]`` (1-based; 0 = never), whatever its metrics are."""

    def __init__(self, stop_after):
        self.stop_after = np.asarray(stop_after)

    def start(self, n):
        from mpi_opt_amd.stopping import StopRule, StopState

        script = self.stop_after

        class State(StopState):
            def update(self, epoch, val_loss, val_acc):
                now = (script == epoch + 1) & ~self.stopped
                self.stopped |= now
                self.stop_epoch[now] = epoch + 1
                return now

        return State(StopRule(), n)


def test_fit_folds_raw_entries_past_the_stopping_epoch_are_nan():
    eng = mnist_engine()
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.uniform(size=(N_SAMPLES, 784)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.randint(0, 10, size=N_SAMPLES).astype(np.int32)).cuda()
    folds = [0, 1, 0, 1, 0, 1]
    stop_after = [1, 0, 2, 3, 0, 1]
    init_params = eng.params.clone()
    runs = {}
    for retire in (False, True):
        eng.params.copy_(init_params)
        eng.reset_optimizer()
        runs[retire] = eng.fit_folds(x, y, folds, 2, 4, stopping=_ScriptedRule(stop_after), retire_stopped=retire)
        assert eng.active.all()                      # the engine comes back with every member active
    plain, ret = runs[False], runs[True]
    assert plain["epochs_run"].tolist() == ret["epochs_run"].tolist() == [1, 4, 2, 3, 4, 1]
    assert np.isfinite(plain["val_loss"]).all()
    for i, e in enumerate(ret["epochs_run"]):
        for key in ("val_loss", "val_acc"):
            assert np.array_equal(ret[key][i, :e], plain[key][i, :e]), (i, key)
            assert np.isnan(ret[key][i, e:]).all(), (i, key)
