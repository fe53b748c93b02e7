"""The DenseNet population (csrc/densenet.hip) against the fp64 oracle at every case of
``tests/dn_cases.py``: the shapes at which the plan changes kernel, instantiation, row
chunking or work split.  The bars are the project's (test_densenet_gpu.py), unchanged:
loss 1e-4 relative, each gradient tensor within 2e-3 of the oracle tensor's max |g|, BN
state rtol 1e-4 / atol 1e-5, trajectory and held-out loss 1e-3, penalty 1e-4.  At these
shapes one lost row or pixel segment is a large share of every sum; the fp32 CPU
restatement uses under 1 % of each bar (test_dn_cases_host.py)."""
import numpy as np
import pytest
import torch

from oracle import densenet as od
from tests import dn_cases as C

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in C.CASES]


def _pop(name, members=(0, 1)):
    """A population of the case's members (by index) and its inputs on the device."""
    from mpi_opt_amd.densenet import DenseNetArch, DenseNetPopulation

    c = C.BY_NAME[name]
    inp = C.inputs(name)
    arch = DenseNetArch(img_dim=c.img, nb_classes=c.classes, depth=c.depth, nb_dense_block=c.blocks,
                        growth_rate=c.growth, nb_filter=c.nbf)
    pop = DenseNetPopulation(arch, [C.LRS[i] for i in members], batch=c.B, init=[inp.init[i] for i in members])
    assert [{k: ly[k] for k in ("kind", "H", "W", "cin", "cout")} for ly in pop.layers] == \
           [{k: ly[k] for k in ("kind", "H", "W", "cin", "cout")} for ly in inp.layers]
    dev = torch.device("cuda")
    order = np.ascontiguousarray(inp.order[list(members)])
    return pop, torch.from_numpy(inp.x).to(dev), torch.from_numpy(inp.y).to(dev), torch.from_numpy(order).to(dev)


def _grads_with_l2(pop, i, init_i):
    dg = pop.get_grads(i)
    return {n: dg[n].astype(np.float64) + 2 * od.L2 * init_i[0][n].astype(np.float64) for n in dg}


def _step0(name, pop, xd, yd, ordd):
    """One train step; {member: {quantity: error as a fraction of its bar}}."""
    ref, inp = C.reference(name), C.inputs(name)
    loss = pop.train_step(xd, yd, ordd, 0).cpu().numpy()
    return {i: C.step0_fractions(float(loss[i]), _grads_with_l2(pop, i, inp.init[i]), pop.get_state(i), ref[i])
            for i in range(len(ref))}


def _report(name, what, fr):
    worst = {i: max(f.items(), key=lambda kv: kv[1]) for i, f in fr.items()}
    print(f"{name} {what}: worst fraction of a bar " + "; ".join(f"member {i} {k} {v:.3g}" for i, (k, v) in worst.items()))
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_one_train_step(name):
    """Loss, every gradient tensor (the 2 L2 w term added back) and the BN moving statistics
    of both members after one step."""
    pop, xd, yd, ordd = _pop(name)
    fr = _step0(name, pop, xd, yd, ordd)
    _report(name, "step 0", fr)
    bad = {(i, k): round(v, 3) for i, f in fr.items() for k, v in f.items() if not v <= 1.0}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", NAMES)
def test_two_more_steps_and_eval(name):
    """Three train steps within the trajectory bar, then one eval_step on a held-out
    batch: val_loss_sum, val_correct (the oracle's count; no sample of the table is
    ambiguous, test_dn_cases_host.py) and the penalty."""
    c, ref = C.BY_NAME[name], C.reference(name)
    pop, xd, yd, ordd = _pop(name)
    B = c.B
    fr = {i: {} for i in range(len(ref))}
    for s in range(C.TRAIN_STEPS):
        dl = pop.train_step(xd, yd, ordd, s * B).cpu().numpy()
        for i, mr in enumerate(ref):
            fr[i][f"loss step {s}"] = abs(dl[i] - mr.losses[s]) / (C.TRAJ_RTOL * abs(mr.losses[s]))
    pop.eval_reset()
    pop.eval_step(xd, yd, ordd, C.TRAIN_STEPS * B)
    vs, vc = pop.val_loss_sum.cpu().numpy(), pop.val_correct.cpu().numpy()
    pen = pop.penalty().cpu().numpy()
    for i, mr in enumerate(ref):
        fr[i]["val_loss_sum"] = abs(vs[i] - mr.eval_sum) / (C.TRAJ_RTOL * abs(mr.eval_sum))
        fr[i]["penalty"] = abs(pen[i] - mr.penalty) / (C.PEN_RTOL * mr.penalty)
    _report(name, "trajectory + eval", fr)
    bad = {(i, k): round(float(v), 3) for i, f in fr.items() for k, v in f.items() if not v <= 1.0}
    assert not bad, (name, bad)
    for i, mr in enumerate(ref):
        # a sample whose two best oracle logits are within 1e-4 may go either way: at most one
        assert mr.eval_ambiguous <= 1
        assert 0 <= int(vc[i]) - mr.eval_correct <= mr.eval_ambiguous, (name, i, int(vc[i]), mr.eval_correct)


@pytest.mark.parametrize("name", ["b65", "w8", "w24"])
def test_member_alone_is_bit_identical(name):
    """Member 1 alone in a population of one: the same parameters and BN state, bit for bit,
    after three steps (two-sample weight-gradient groups and 65 fused slices at B = 65; the
    fused reduce at W = 8 and 4; the ragged chunks and slices of the 24-wide case)."""
    c = C.BY_NAME[name]
    full, xd, yd, ordd = _pop(name)
    solo, _, _, ord1 = _pop(name, members=(1,))
    for s in range(C.TRAIN_STEPS):
        full.train_step(xd, yd, ordd, s * c.B)
        solo.train_step(xd, yd, ord1, s * c.B)
    torch.cuda.synchronize()
    assert torch.equal(full.params[1], solo.params[0])
    assert torch.equal(full.state[1], solo.state[0])


@pytest.mark.parametrize("name", ["ref16", "w8"])
def test_plan_switches(name, monkeypatch):
    """MPO_DN_PLAN: wg2=0 and wgs=3 only move weight gradients between streams (bit-identical
    gradients, parameters and state after two steps); bnfuse=0 runs the BN backward reduce
    as its own pass: gradients within 1e-5 of the tensor max of the default's (the bar of
    the c1x1=0 test) and itself within the oracle bars."""
    c = C.BY_NAME[name]
    out = {}
    for plan in ("", "wg2=0", "wgs=3", "bnfuse=0"):
        if plan:
            monkeypatch.setenv("MPO_DN_PLAN", plan)
        else:
            monkeypatch.delenv("MPO_DN_PLAN", raising=False)
        pop, xd, yd, ordd = _pop(name)
        fr = _step0(name, pop, xd, yd, ordd)
        g0 = pop.grads.clone()
        pop.train_step(xd, yd, ordd, c.B)
        torch.cuda.synchronize()
        out[plan] = (g0, pop.grads.clone(), pop.params.clone(), pop.state.clone(), fr)
    for plan in ("wg2=0", "wgs=3"):
        for a, b in zip(out[""][:4], out[plan][:4]):
            assert torch.equal(a, b), plan
    ga, gb = out[""][0], out["bnfuse=0"][0]
    assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())
    fr = out["bnfuse=0"][4]
    _report(name, "bnfuse=0 step 0", fr)
    bad = {(i, k): round(v, 3) for i, f in fr.items() for k, v in f.items() if not v <= 1.0}
    assert not bad, (name, bad)


def test_arena_stays_clean_at_a_suspect_width():
    """After a step at W = 24 (an m-tile straddles two image rows there): the whole arena
    is finite, the BN totals region holds the head site's per-row (sum, sum of squares)
    of every member -- within 1e-4 of the row's sum of magnitudes / of squares, the
    relative bar of the BN state on the sums the statistics are made of -- and every
    member's BN state is the oracle's.  A store past the slice partials lands here."""
    name = "w24"
    c, ref = C.BY_NAME[name], C.reference(name)
    pop, xd, yd, ordd = _pop(name)
    pop.train_step(xd, yd, ordd, 0)
    torch.cuda.synchronize()
    ar = C.arena(c, len(ref))
    assert ar["act_floats"] == pop.act.numel()
    act = pop.act.cpu().numpy()
    assert np.isfinite(act).all()
    assert np.isfinite(pop.params.cpu().numpy()).all() and np.isfinite(pop.state.cpu().numpy()).all()
    Hh = pop.layers[-1]["H"]
    hmax = max(ly["H"] for ly in pop.layers)
    region = act[ar["bnt"]:ar["bnt"] + len(ref) * ((4 * hmax + 63) & ~63)].view(np.float64)
    tot = region[:len(ref) * Hh * 2].reshape(len(ref), Hh, 2)
    for i, mr in enumerate(ref):
        assert np.all(np.abs(tot[i, :, 0] - mr.head_tot[:, 0]) <= C.STATE_RTOL * mr.head_tot[:, 2]), (i, tot[i], mr.head_tot)
        assert np.all(np.abs(tot[i, :, 1] - mr.head_tot[:, 1]) <= C.STATE_RTOL * mr.head_tot[:, 1]), (i, tot[i], mr.head_tot)
        st = pop.get_state(i)
        for n, v in mr.state0.items():
            np.testing.assert_allclose(st[n], v, rtol=C.STATE_RTOL, atol=C.STATE_ATOL, err_msg=n)
    # and the slice partials past the widest site's slices are untouched (zero since allocation)
    bnp = act[ar["bnp"]:ar["bnt"]].view(np.float64)
    assert not bnp[len(ref) * ar["bnp_doubles"]:].any(), "a store past the BN slice partials"
