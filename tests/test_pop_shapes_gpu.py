"""GPU parity of the MNIST population engine (csrc/cnn.hip) with the fp64 oracle
(oracle/cnn.py) on every plan path, batch and ABI edge of ``tests/pop_cases.py``:
eval forward, step-0 loss, activations, discrete decisions and every gradient tensor,
three more steps of losses, and that a step writes only the floats it owns.

No tolerance here is new: 1e-5 (loss), ``1e-4 max + 2e-5 sum|terms|`` (tensors) and
1e-3 (trajectory) are tests/test_train_gpu.py's bars for this engine."""
import numpy as np
import pytest
import torch

from tests import pop_cases as C

pytestmark = pytest.mark.gpu

LOSS_REL, TRAJ_REL = 1e-5, 1e-3
MPO_ENOTSUP = 3   # include/mpo.h


def tensor_bound(ref, abs_terms):
    """f32 bound of test_train_gpu.py: 1e-4 of the tensor's scale plus 2e-5 of the sum
    of |terms| of the entry's contraction."""
    return 1e-4 * np.abs(ref).max() + 2e-5 * abs_terms


def in_units(err, bound):
    """The largest err / bound; an entry whose bound is 0 (no terms) must be exact."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def make_engine(name, only=None):
    from mpi_opt_amd.population import PopulationEngine, TrialSpec

    B, members = C.POP[name]
    ref = C.reference(name)
    idx = range(len(members)) if only is None else only
    specs = [TrialSpec(members[i].F, members[i].k, members[i].p, members[i].dense, members[i].lr, members[i].dropout,
                       seed=ref.members[i].seed, loss=members[i].loss, optimizer=members[i].optimizer) for i in idx]
    return PopulationEngine(specs, batch=B, init=[ref.members[i].init for i in idx]), specs


def owned_mask(eng):
    """True for every float of the parameter arena inside a member's tensor."""
    own = np.zeros(eng.n_params, dtype=bool)
    for i in range(eng.n):
        for off, shape in eng._slices(i).values():
            own[off:off + int(np.prod(shape))] = True
        assert eng.layout[i][8] <= eng.n_params
    return own


def check_population(name):
    """Every check of one population on one engine.  Returns (failures, units): the
    failed checks by name, and the largest error of each kind in units of its bound."""
    B, members = C.POP[name]
    ref = C.reference(name)
    eng, specs = make_engine(name)
    xd, yd = torch.from_numpy(ref.x).cuda(), torch.from_numpy(ref.y).cuda()
    otr, ova = torch.from_numpy(ref.train).cuda(), torch.from_numpy(ref.val).cuda()
    fails, units, flips = [], {}, {}

    def unit(kind, value, who):
        units[kind] = max(units.get(kind, 0.0), float(value))
        if not value <= 1.0:
            fails.append(f"{who} {kind}: {float(value):.3g} units")

    # ---- eval forward of one batch
    eng.eval_reset()
    eng.eval_step(xd, yd, ova, 0)
    ev_loss = eng.val_loss_sum.cpu().numpy() / B
    ev_hits = eng.val_correct.cpu().numpy()
    for i, mr in enumerate(ref.members):
        unit("eval_loss", abs(ev_loss[i] - mr.eval_loss) / (LOSS_REL * abs(mr.eval_loss)), f"{name}/{i}")
        if abs(int(ev_hits[i]) - mr.eval_hits) > mr.eval_close:
            fails.append(f"{name}/{i} val_correct {int(ev_hits[i])} vs {mr.eval_hits} ({mr.eval_close} near ties)")

    # ---- train step 0: loss, activations, decisions, gradients
    loss = eng.train_step(xd, yd, otr, 0).cpu().numpy().copy()
    grads = eng.grads.cpu().numpy()
    for i, (mr, s) in enumerate(zip(ref.members, specs)):
        who = f"{name}/{i}"
        m, g, cache = mr.member, s.geometry(), mr.cache
        unit("loss", abs(loss[i] - mr.loss0) / (LOSS_REL * abs(mr.loss0)), who)
        shapes = {"a1": (B, g["H1"], g["H1"], m.F), "a2": (B, g["H2"], g["H2"], m.F), "pd": (B, g["K1"]),
                  "h": (B, m.dense)}
        dev = {t: eng.activation(i, t, shape) for t, shape in shapes.items()}
        # decisions first: an activation may differ by a whole entry only where its decision may
        dec = {"arg": eng.argmax_table(i).reshape(B, g["s"], g["s"], m.F).astype(np.int64)}
        free = mr.ambig["arg"] | mr.ambig["dead"]
        bad = (dec["arg"] != cache["arg"]) & ~free
        flips[who] = {"arg": int(np.sum((dec["arg"] != cache["arg"]) & ~mr.ambig["dead"]))}
        if bad.any():
            fails.append(f"{who} argmax: {int(bad.sum())} of {bad.size} windows differ outside the ambiguous set")
        for t in ("a1", "a2", "h"):
            dec[t + "_pos"] = dev[t] > 0
            diff = dec[t + "_pos"] != (cache[t] > 0)
            flips[who][t] = int(diff.sum())
            if (diff & ~mr.ambig[t]).any():
                fails.append(f"{who} {t} > 0: {int((diff & ~mr.ambig[t]).sum())} of {diff.size} gates differ outside "
                             f"the ambiguous set")
        for t in shapes:
            err = np.abs(dev[t] - cache[t].reshape(shapes[t]))
            unit("act " + t, in_units(err, tensor_bound(cache[t], mr.abs_act[t].reshape(shapes[t]))), who)
        o = C.make_oracle(m, mr.seed, mr.init)
        gr, absg = o.backward(cache, abs_terms=True, decisions=dec)
        for pname, (off, shape) in eng._slices(i).items():
            gd = grads[off:off + int(np.prod(shape))].reshape(shape)
            unit("grad " + pname, in_units(np.abs(gd - gr[pname]), tensor_bound(gr[pname], absg[pname])), who)

    # ---- three more steps: step_count runs, row0 advances
    for st in range(1, C.TRAIN_STEPS):
        loss = eng.train_step(xd, yd, otr, st * B).cpu().numpy()
        for i, mr in enumerate(ref.members):
            unit("trajectory", abs(loss[i] - mr.losses[st]) / (TRAJ_REL * abs(mr.losses[st])), f"{name}/{i} step {st}")

    # ---- ownership: the 64-float padding between the tensors is never written
    own = owned_mask(eng)
    for arena in ("params", "grads", "adam_m", "adam_v"):
        a = getattr(eng, arena).cpu().numpy()
        n_bad = int(np.count_nonzero(a[~own]))
        if n_bad:
            fails.append(f"{name} {arena}: {n_bad} floats outside the members' tensors are not 0.0")
    return fails, units, flips


def report(name, fails, units, flips):
    print(f"{name}: " + "  ".join(f"{k} {v:.2g}" for k, v in units.items()))
    print(f"{name}: decisions that differ (all inside the ambiguous set unless listed below): "
          + "  ".join(f"{who} {d}" for who, d in flips.items() if any(d.values())))
    for f in fails:
        print("FAIL", f)


@pytest.mark.parametrize("name", [n for n, _, _ in C.POPULATIONS])
def test_population_matches_oracle(name):
    fails, units, flips = check_population(name)
    report(name, fails, units, flips)
    assert not fails, fails


def test_isolation_at_a_batch_the_sample_groups_do_not_divide():
    """B = 5: conv1 slabs of 2 + 3 samples, conv2 slabs of 2 + 3 (4 per slab) or
    1 + 2 + 2.  One member stepped alone gives the loss bits it has in the population."""
    name, i = "b5", 4
    B, members = C.POP[name]
    cl = C.classes(*members[i][:4], B)
    assert not cl["g1_even"] and not cl["g2_even"] and cl["spg2"] == 4
    ref = C.reference(name)
    xd, yd = torch.from_numpy(ref.x).cuda(), torch.from_numpy(ref.y).cuda()
    eng_all, _ = make_engine(name)
    eng_one, _ = make_engine(name, only=[i])
    for st in range(3):
        la = eng_all.train_step(xd, yd, torch.from_numpy(ref.train).cuda(), st * B).cpu().numpy()
        lo = eng_one.train_step(xd, yd, torch.from_numpy(ref.train[i:i + 1]).cuda(), st * B).cpu().numpy()
        assert la[i] == lo[0], (st, la[i], lo[0])


def test_shapes_past_the_accepted_domain_are_refused():
    """kernel_size > 10 and pool_size > 16 return MPO_ENOTSUP with the member and the
    reason, at the first refused values (pop_cases.REFUSED records what each computed
    while it was accepted); the last accepted values, k = 10 and p = 16, plan here and
    pass parity in the table above (b1/0, b2/3, b64/2; b2/4, b3/0)."""
    import ctypes

    from mpi_opt_amd import _lib

    for name, B, (m,) in C.REFUSED:
        arr = (_lib.MpoCnnSpec * 2)()
        arr[0] = _lib.MpoCnnSpec(8, 10, 10, 20, 1e-3, 0.25, 1, 0)
        arr[1] = _lib.MpoCnnSpec(m.F, m.k, m.p, m.dense, 1e-3, 0.25, 1, 0)
        h = ctypes.c_void_p()
        assert _lib.lib().mpo_pop_create(arr, 2, B, ctypes.byref(h)) == MPO_ENOTSUP, name
        msg = _lib.lib().mpo_last_error().decode()
        assert "member 1" in msg and ("kernel_size" if m.k > C.K_MAX else "pool_size") in msg, msg
    for F, k, p in [(8, 10, 10), (8, 2, 16)]:
        arr = (_lib.MpoCnnSpec * 1)()
        arr[0] = _lib.MpoCnnSpec(F, k, p, 20, 1e-3, 0.25, 1, 0)
        h = ctypes.c_void_p()
        assert _lib.lib().mpo_pop_create(arr, 1, 3, ctypes.byref(h)) == 0, (F, k, p)
        _lib.lib().mpo_pop_destroy(h)
