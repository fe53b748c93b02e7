"""GPU parity of the topclass population engine (csrc/topclass.hip) against the fp64 numpy
reference tests/topclass_ref.py on identical seeded weights, data order and dropout masks.
Bars: the MNIST engine's (tests/test_train_gpu.py) -- one-step loss 1e-5 relative, every
gradient tensor within 1e-4 max|g| + 2e-5 sum|terms|; trajectories 1e-3 relative."""
import numpy as np
import pytest
import torch

from tests import topclass_cases as TC
from tests import topclass_ref as R

pytestmark = pytest.mark.gpu


def build(case, members=None):
    """(engine, specs, init, x, y): member i of the case has dropout seed 1000 + i and init seed 7 + i."""
    from mpi_opt_amd.topclass import TopclassPopulation, TopclassSpec, glorot_uniform_init

    idx = list(range(len(case.members))) if members is None else list(members)
    specs = [TopclassSpec(kernel_size=case.members[i][0], dropout=case.members[i][1], lr=(1e-3, 2e-3, 5e-2)[i % 3]
                          if case.members[i][3] == "adam" else 5e-2, seed=1000 + i, input_shape=case.shape,
                          classes=case.classes, loss=case.members[i][2], optimizer=case.members[i][3]) for i in idx]
    rng = np.random.RandomState(3)
    init = []
    for i, s in zip(idx, specs):
        p = glorot_uniform_init(s, 7 + i)
        for n in ("b1", "b2", "b3", "b4"):      # non-zero biases: the bias adds are under test too
            p[n] = np.random.RandomState(70 + i).uniform(-0.1, 0.1, size=p[n].shape).astype(np.float32)
        init.append(p)
    n = case.n_samples or case.batch
    x = rng.uniform(size=(n,) + tuple(case.shape)).astype(np.float32)
    y = rng.randint(0, case.classes, size=n).astype(np.int32)
    eng = TopclassPopulation(specs, batch=case.batch, init=init)
    return eng, specs, init, x, y


def reference(case, spec, params):
    return R.TopclassRef(case.shape, case.classes, spec.kernel_size, {n: v.astype(np.float64) for n, v in params.items()},
                         lr=spec.lr, dropout=spec.dropout, seed=spec.seed, loss=spec.loss, optimizer=spec.optimizer)


def orders(eng, n, shift=True):
    """Member i reads the samples rotated by i (every member its own order row)."""
    o = np.stack([np.roll(np.arange(n, dtype=np.int32), -i if shift else 0) for i in range(eng.n)])
    return o, torch.from_numpy(o).cuda()


def decisions(eng, i, spec):
    """The device forward's discrete choices (pool argmax, ReLU gates) of member i."""
    g, B = spec.geometry(), eng.batch
    return {"arg": eng.activation(i, "am", (B, g["Hp"], g["Wp"], 32), torch.int32).astype(np.int64),
            "a1_pos": eng.activation(i, "a1", (B, g["H1"], g["W1"], 32)) > 0,
            "a2_pos": eng.activation(i, "a2", (B, g["H2"], g["W2"], 32)) > 0,
            "h_pos": eng.activation(i, "h", (B, 128)) > 0}


def check_step(case, eng, specs, refs, x, y, o, row0, step, loss):
    report = []
    for i, s in enumerate(specs):
        rows = o[i][row0:row0 + case.batch]
        ref_loss, _, _, cache = refs[i].forward(x[rows], y[rows], step=step, train=True)
        g, absg = refs[i].backward(cache, abs_terms=True, decisions=decisions(eng, i, s))
        print("%s member %d k=%d loss %.8g ref %.8g" % (case.name, i, s.kernel_size, loss[i], ref_loss))
        assert abs(loss[i] - ref_loss) <= 1e-5 * abs(ref_loss), (case.name, i, loss[i], ref_loss)
        gd = eng.get_grads(i)
        for name in g:
            err = np.abs(gd[name] - g[name])
            bound = 1e-4 * np.abs(g[name]).max() + 2e-5 * absg[name]
            report.append((i, name, float((err / (np.abs(g[name]).max() + 1e-30)).max()),
                           float((err / (absg[name] + 1e-30)).max()), bool(np.all(err <= bound))))
    for r in report:
        print("%s member %d %-3s err/max %.2e err/sum|terms| %.2e ok=%s" % ((case.name,) + r))
    assert all(r[-1] for r in report), case.name


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.name)
def test_one_step_loss_and_gradients_match_reference(case):
    eng, specs, init, x, y = build(case)
    o, od = orders(eng, x.shape[0])
    loss = eng.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), od, 0, step=0).cpu().numpy()
    refs = [reference(case, s, init[i]) for i, s in enumerate(specs)]
    check_step(case, eng, specs, refs, x, y, o, 0, 0, loss)


def test_second_step_gradients_match_reference():
    """The buffers are reused: conv2's input gradient must write exact zeros to the a1 pixels no
    window reaches (k = 1) on every step.  The reference starts the second step from the
    device's own parameters after the first."""
    case = TC.SECOND_STEP
    eng, specs, init, x, y = build(case)
    o, od = orders(eng, x.shape[0])
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    eng.train_step(xd, yd, od, 0, step=0)
    refs = [reference(case, s, eng.get_params(i)) for i, s in enumerate(specs)]
    loss = eng.train_step(xd, yd, od, case.batch, step=1).cpu().numpy()
    check_step(case, eng, specs, refs, x, y, o, case.batch, 1, loss)
    g = specs[0].geometry()                  # k = 1: a1 rows / columns 1, 2 (mod 3) are in no conv2 window
    dz1 = eng.activation(0, "dz1", (case.batch, g["H1"], g["W1"], 32))
    assert np.all(dz1[:, 1::3] == 0) and np.all(dz1[:, 2::3] == 0) and np.all(dz1[:, :, 1::3] == 0)
    assert np.any(dz1[:, 0::3, 0::3] != 0)


def test_trajectory_matches_reference():
    case = TC.TRAJECTORY
    eng, specs, init, x, y = build(case)
    o, od = orders(eng, x.shape[0])
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    B, steps = case.batch, 6
    got = np.stack([eng.train_step(xd, yd, od, st * B).cpu().numpy().copy() for st in range(steps)], 1)
    eng.eval_reset()
    eng.eval_step(xd, yd, od, steps * B)
    vl, vc = eng.val_loss_sum.cpu().numpy(), eng.val_correct.cpu().numpy()
    for i, s in enumerate(specs):
        ref = reference(case, s, init[i])
        want = [ref.train_step(x[o[i][st * B:(st + 1) * B]], y[o[i][st * B:(st + 1) * B]], st) for st in range(steps)]
        rows = o[i][steps * B:(steps + 1) * B]
        rl, rc = ref.eval_batch(x[rows], y[rows])
        print("member %d train %s ref %s val %.8g ref %.8g correct %d ref %d" % (i, got[i], np.array(want), vl[i], rl,
                                                                               vc[i], rc))
        assert np.all(np.abs(got[i] - want) <= 1e-3 * np.abs(want)), (i, got[i], want)
        assert abs(vl[i] - rl) <= 1e-3 * abs(rl) and int(vc[i]) == rc, (i, vl[i], rl, vc[i], rc)


@pytest.mark.parametrize("case,member", TC.ISOLATION, ids=lambda v: getattr(v, "name", str(v)))
def test_member_bits_do_not_depend_on_the_population(case, member):
    def run(members):
        eng, specs, init, x, y = build(case, members)
        row = np.arange(x.shape[0], dtype=np.int32)
        od = torch.from_numpy(np.stack([row] * eng.n)).cuda()
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        j = list(members).index(member)
        losses = [eng.train_step(xd, yd, od, st * case.batch)[j].item() for st in range(3)]
        return losses, eng.get_params(j)

    alone_l, alone_p = run([member])
    pop_l, pop_p = run(range(len(case.members)))
    assert alone_l == pop_l and all(np.isfinite(alone_l))
    for n in alone_p:
        assert np.array_equal(alone_p[n], pop_p[n]), n


def _small_problem():
    from mpi_opt_amd.topclass import synthetic_topclass

    return synthetic_topclass(60, shape=(30, 26, 5), classes=3, seed=1, device="cuda", labels="learnable")


def test_trial_evaluator_routes_test_cnn_specs():
    from mpi_opt_amd.blocks import TrialEvaluator
    from mpi_opt_amd.search import example_provider

    x, y = _small_problem()
    assert x.shape == (60, 30, 26, 5) and y.dtype == torch.int32 and int(y.max()) <= 2
    provider = example_provider("topclass", (30, 26, 5))
    trials, ids = [[0.3, 2, 5.0], [1.0, 4, 2.0], [0.0, 1, 9.0]], [11, 5, 42]

    def foms(order):
        ev = TrialEvaluator(provider, x, y, n_fold=2, epochs=2, batch=10, loss="categorical_crossentropy")
        out = ev.evaluate([trials[i] for i in order], trial_ids=[ids[i] for i in order])
        return {order[j]: out[j] for j in range(len(order))}

    a, b = foms([0, 1, 2]), foms([2, 0, 1])
    assert all(np.isfinite(v) and 0 < v < 20 for v in a.values())
    assert a == b


def test_topclass_search_end_to_end(tmp_path, monkeypatch):
    import random

    from mpi_opt_amd import search

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    x, y = _small_problem()
    args = search.make_parser().parse_args(
        ["--example", "topclass", "--world-size", "3", "--block-size", "2", "--epochs", "1", "--num-iterations", "2",
         "--batch", "10", "--ei-candidates", "200", "--loss", "categorical_crossentropy"])
    rep = search.run_search(args, x=x, y=y, log=lambda *a: None)
    assert rep["trials_told"] >= 1 and rep["trials_trained"] >= rep["trials_told"]
