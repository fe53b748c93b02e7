"""tests/topclass_ref.py (the fp64 reference of the topclass GPU tests) against torch
autograd on the CPU: F.conv2d(stride=3), F.max_pool2d, fp64, the same dropout masks applied
as fixed multipliers; loss and every gradient to 1e-10 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import topclass_ref as R

# (H, W, C, k, classes, B, dropout, loss): k in {1, 2, 3, 4, 7}; (in - k) % 3 in {0, 1, 2} on
# either convolution; odd conv2 outputs (the pool drops a row / column); both losses
CASES = [
    (13, 16, 5, 1, 3, 3, 0.3, "categorical_crossentropy"),
    (20, 14, 1, 2, 5, 2, 1.0, "binary_crossentropy"),
    (19, 21, 5, 3, 3, 4, 0.0, "categorical_crossentropy"),
    (30, 26, 3, 3, 3, 2, 0.5, "binary_crossentropy"),          # conv2 output 3 x 2: the pool drops a row
    (24, 29, 5, 4, 3, 3, 0.3, "binary_crossentropy"),
    (43, 40, 2, 7, 4, 2, 0.6, "categorical_crossentropy"),     # k > 2 strides: overlapping windows
]


def test_cases_cover_every_residue():
    res = {"c1h": set(), "c1w": set(), "c2h": set(), "c2w": set()}
    odd = False
    for (H, W, C, k, *_rest) in CASES:
        g = R.geometry((H, W, C), k)
        res["c1h"].add((H - k) % 3); res["c1w"].add((W - k) % 3)
        res["c2h"].add((g["H1"] - k) % 3); res["c2w"].add((g["W1"] - k) % 3)
        odd |= g["H2"] % 2 == 1 or g["W2"] % 2 == 1
    assert all(v == {0, 1, 2} for v in res.values()), res
    assert odd and {c[3] for c in CASES} == {1, 2, 3, 4, 7} and {c[7] for c in CASES} == set(R.LOSSES)


def torch_loss(P, x, y, m1, m2, classes, loss):
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    w = {n: t(v).requires_grad_(True) for n, v in P.items()}
    h = F.relu(F.conv2d(t(x).permute(0, 3, 1, 2), w["w1"].permute(3, 2, 0, 1), w["b1"], stride=3))
    h = F.relu(F.conv2d(h, w["w2"].permute(3, 2, 0, 1), w["b2"], stride=3))
    h = F.max_pool2d(h, 2)
    flat = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1) * t(m1)     # NHWC flatten
    hd = F.relu(flat @ w["w3"] + w["b3"]) * t(m2)
    p = torch.softmax(hd @ w["w4"] + w["b4"], dim=1)
    oh = F.one_hot(torch.tensor(y, dtype=torch.int64), classes).to(torch.float64)
    if loss == "binary_crossentropy":
        pc = torch.clamp(p, R.EPS, 1 - R.EPS)
        l = (-(oh * torch.log(pc) + (1 - oh) * torch.log(1 - pc))).mean(dim=1).mean()
    else:
        q = p / p.sum(dim=1, keepdim=True)
        l = (-torch.log(torch.clamp((q * oh).sum(dim=1), R.EPS, 1 - R.EPS))).mean()
    l.backward()
    return float(l.detach()), {n: v.grad.numpy() for n, v in w.items()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "H%dW%dC%dk%d" % c[:4])
def test_reference_matches_torch_autograd(case):
    H, W, C, k, classes, B, dropout, loss = case
    from mpi_opt_amd.topclass import TopclassSpec, glorot_uniform_init

    spec = TopclassSpec(kernel_size=k, dropout=dropout, input_shape=(H, W, C), classes=classes, loss=loss)
    g = spec.geometry()
    assert g == R.geometry((H, W, C), k)
    rng = np.random.RandomState(k)
    P = {n: v.astype(np.float64) for n, v in glorot_uniform_init(spec, 5).items()}
    for n in ("b1", "b2", "b3", "b4"):
        P[n] = rng.uniform(-0.1, 0.1, size=P[n].shape)
    x = rng.uniform(size=(B, H, W, C))
    y = rng.randint(0, classes, size=B)
    ref = R.TopclassRef((H, W, C), classes, k, P, dropout=dropout, seed=11, loss=loss)
    loss_ref, _, _, cache = ref.forward(x, y, step=2, train=True)
    grads, absg = ref.backward(cache, abs_terms=True)
    r0, r1 = R.dropout_rates(dropout)
    assert (r0 is None) == (dropout in (0.0,)) and (r1 is None) == (dropout in (0.0, 1.0))
    if r0 is not None:
        assert set(np.unique(cache["m1"])) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(r0)))}
    loss_t, grads_t = torch_loss(P, x, y, cache["m1"], cache["m2"], classes, loss)
    assert abs(loss_ref - loss_t) <= 1e-10 * abs(loss_t)
    for n in P:
        scale = np.abs(grads_t[n]).max()
        assert scale > 0 and np.abs(grads[n] - grads_t[n]).max() <= 1e-10 * scale, n
        assert np.all(absg[n] >= np.abs(grads[n]) - 1e-12 * scale), n


def test_update_rules_are_the_oracles():
    """Adam / SGD of the reference are oracle/cnn.py's TrialOracle rules."""
    from oracle import cnn as OC

    rng = np.random.RandomState(0)
    shapes = dict(OC.param_shapes(4, 3, 2, 8))
    P = {n: rng.standard_normal(s) for n, s in shapes.items()}
    for opt in ("adam", "sgd"):
        o = OC.TrialOracle(4, 3, 2, 8, P, lr=float(np.float32(3e-3)), optimizer=opt)
        r = R.TopclassRef((20, 20, 1), 3, 3, P, lr=3e-3, optimizer=opt)
        for _ in range(3):
            G = {n: rng.standard_normal(s) for n, s in shapes.items()}
            (o.adam if opt == "adam" else o.sgd)(G)
            r.update(G)
        for n in P:
            assert np.array_equal(o.params[n], r.params[n]), (opt, n)


def test_input_gradient_zero_where_no_window_reaches():
    """k < 3 leaves a1 pixels in no conv2 window; trailing (in - k) % 3 rows are never read."""
    rng = np.random.RandomState(1)
    w = rng.standard_normal((2, 2, 3, 4))
    dz = rng.standard_normal((1, 3, 2, 4))
    dx = R.conv_dgrad(dz, (1, 10, 6, 3), w)
    assert np.all(dx[:, 2::3] == 0) and np.all(dx[:, :, 2::3] == 0) and np.all(dx[:, 8:] == 0)
    assert np.all(dx[:, 0:8:3, 0:5:3] != 0)
