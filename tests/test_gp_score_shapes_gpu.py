"""GPU parity of GP scoring over the case table of ``tests/score_cases.py``: every
instance of ``gp_score_kernel`` and ``gp_score_streamed_kernel`` with one tile per
workgroup and looped, the wave-plan edges, the resident/streamed boundary at the
narrowest and widest width, every top-k width, ties from underflow, and the Matern's
hand-written exp / sqrt over scaled distances from 0 to 1e19.

Every case is held to the project's bars (tests/test_gp_gpu.py): mu within 1e-9 of its
summand scale and sd within 1e-9 relative of the 80-bit posterior (the fp64 triangular
form past n = 600); acquisition values within rtol 1e-10 / atol 1e-300 of the oracle on
the device's own posterior; top-k equal to the reference's (gaps checked on the host);
``val == values[idx]`` bit for bit.  Each case first asserts the path it claims to take.
On top of that, per class: looped cases are rescored one tile per workgroup (mu
bit-equal, sd^2 within 8 eps amp y_std^2) and repeated (bit-equal); a model scored on
both paths agrees within 1e-10; the K* cases hold mu to one unit of
``score_cases.kstar_reference`` -- gp.hip's own 2-ulp claims for exp_neg and sqrt_pos.

Each case prints its errors as fractions of its bars (``-s`` shows them; DESIGN §4
records a run)."""
import ctypes

import numpy as np
import pytest
import torch

from mpi_opt_amd import _lib
from oracle import gp_ei as O
from tests import score_cases as C

pytestmark = pytest.mark.gpu

EPS = C.EPS


def set_env(monkeypatch, c):
    for name, v in (("MPO_GP_SCORE", c.score), ("MPO_GP_PANEL", c.panel if c.score == "streamed" else None),
                    ("MPO_GP_DIST", c.dist)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def xb_flag(g):
    """The expanded-distance device flag of a prepared model (None without xb)."""
    m = g.model
    if not m.xb:
        return None
    off = m.xb + (m.np16 + 32) * m.dp * 8 - g._ws.data_ptr()
    return float(g._ws[off:off + 8].cpu().numpy().view(np.float64)[0])


def build(c, p, monkeypatch):
    """The case's model under the case's switches, after asserting that it is scored
    the way score_cases.facts says."""
    from mpi_opt_amd.gp import DeviceGP

    set_env(monkeypatch, c)
    f = C.facts(c)
    g = DeviceGP(p.X, p.y, p.st.amp, p.st.length_scale, p.st.noise)
    assert g.score_path == f["path"], c.name
    assert (g.model.dp, g.model.np16, g.model.d) == (f["dp"], f["np16"], c.d)
    assert bool(g.model.xb) == f["xb"], c.name
    flag = xb_flag(g)
    if f["form"] == "md":
        # every model row and every candidate tile is inside the guard: the MFMA distance runs
        assert flag == 1.0, c.name
        assert np.max(np.sum((p.C / p.st.length_scale) ** 2, axis=1)) <= C.K_DIST_NORM
    elif f["form"] == "guarded":
        assert flag in (0.0, 1.0)
        if np.max(np.sum((p.X / p.st.length_scale) ** 2, axis=1)) > C.K_DIST_NORM:
            assert flag == 0.0, c.name             # a model row outside the guard: the kernel takes the direct form
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt = -(-f["m"] // C.K_BM)
    if f["looped"]:
        assert nt // min(nt, f["cap"], 8 * cus) >= 2, c.name     # every workgroup loops
    if f["one_tile"]:
        assert nt <= cus, c.name                   # one tile per workgroup
    return g


def score(g, c, p, Cd=None):
    Cd = torch.tensor(p.C, device="cuda") if Cd is None else Cd
    out = g.score(Cd, p.y_opt, acqs=C.ACQS, k=c.k)
    torch.cuda.synchronize()
    return out


def check_outputs(c, p, out, mu_bar=True):
    """The bars every case is held to.  Returns (mu, sd) as numpy.  mu_bar = False (the K*
    cases): mu is held to kstar_reference's unit instead -- with y_mean = 0 the summand
    scale falls through the denormals with K*, where one ulp is more than 1e-9 of it."""
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    m = len(p.C)
    assert mu.shape == (m,) and np.all(np.isfinite(mu)) and np.all(np.isfinite(sd))
    d_mu = np.abs(mu[p.sel] - p.mu_ref)
    d_sd = np.abs(sd[p.sel] - p.sd_ref)
    ok = p.scale > (0.0 if mu_bar else 1e-290)
    e_mu = float(np.max(d_mu[ok] / p.scale[ok]))
    e_sd = float(np.max(d_sd / np.maximum(p.sd_ref, 1e-300)))
    print(f"SCORE-CASE {c.name} [{'; '.join(C.classes_of(c))}]: mu {e_mu / 1e-9:.2e} of its bar, sd {e_sd / 1e-9:.2e}")
    assert not mu_bar or np.all(d_mu <= 1e-9 * p.scale), (c.name, e_mu)
    assert np.all(d_sd <= 1e-9 * p.sd_ref), (c.name, e_sd)
    for acq in C.ACQS:
        v = out["values"][acq].cpu().numpy()
        assert np.all(np.isfinite(v)), (c.name, acq)
        np.testing.assert_allclose(v, O.acquisition_values(mu, sd, p.y_opt, acq), rtol=1e-10, atol=1e-300,
                                   err_msg=f"{c.name} {acq}")
        if c.k == 0:
            continue
        idx, val = (t.cpu().numpy() for t in out["topk"][acq])
        assert idx.shape == (c.k,)
        kk = min(c.k, m)
        mode = C.topk_mode(c, acq)
        want = (O.topk_lowest(p.values[acq], kk) if mode == "ref" else np.arange(kk) if mode == "zeros"
                else np.argsort(v, kind="stable")[:kk])
        np.testing.assert_array_equal(idx[:kk], want, err_msg=f"{c.name} {acq} ({mode})")
        assert np.all(idx[kk:] == -1), (c.name, acq)
        np.testing.assert_array_equal(val[:kk].view(np.int64), v[idx[:kk]].view(np.int64), err_msg=f"{c.name} {acq}")
    return mu, sd


def check_looped(g, c, p, out, Cd):
    """Position independence and repeatability of a looped launch (test_gp_score_tiles_gpu.py)."""
    st = p.st
    m = Cd.shape[0]
    chunk = 16 * torch.cuda.get_device_properties(0).multi_processor_count     # one tile per workgroup
    mu_c, sd_c = [], []
    for s in range(0, m, chunk):
        o = g.score(Cd[s:s + chunk], p.y_opt, acqs=C.ACQS, k=c.k)
        mu_c.append(o["mu"])
        sd_c.append(o["sd"])
    mu_c, sd_c = torch.cat(mu_c), torch.cat(sd_c)
    dvar = float(torch.max(torch.abs(out["sd"] ** 2 - sd_c ** 2)))
    bad = int(torch.count_nonzero(out["mu"] != mu_c))
    unit = EPS * st.amp * st.y_std ** 2
    print(f"SCORE-LOOP {c.name}: chunked mu rows differing {bad}, max |dvar| {dvar / unit:.2f} eps amp y_std^2 (bar 8)")
    assert torch.equal(out["mu"], mu_c), c.name
    assert dvar <= 8 * unit, c.name


def check_repeat(g, c, p, out, Cd):
    again = score(g, c, p, Cd)
    assert torch.equal(out["mu"], again["mu"]) and torch.equal(out["sd"], again["sd"]), c.name
    for acq in C.ACQS:
        assert torch.equal(out["values"][acq], again["values"][acq]), (c.name, acq)
        if c.k:
            assert torch.equal(out["topk"][acq][0], again["topk"][acq][0]), (c.name, acq)
            assert torch.equal(out["topk"][acq][1], again["topk"][acq][1]), (c.name, acq)


def check_other_path(c, p, out, monkeypatch):
    """The same model on the other scoring path: 1e-10 on mu's scale and on sd, equal top-k."""
    other = c._replace(score=None, panel=None) if c.score == "streamed" else c._replace(score="streamed")
    assert C.facts(other)["path"] != C.facts(c)["path"]
    g2 = build(other, p, monkeypatch)
    o2 = score(g2, other, p)
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    mu2, sd2 = o2["mu"].cpu().numpy(), o2["sd"].cpu().numpy()
    e_mu = float(np.max(np.abs(mu - mu2)[p.sel] / p.scale))
    e_sd = float(np.max(np.abs(sd - sd2) / sd))
    print(f"SCORE-PATHS {c.name}: resident vs streamed mu {e_mu / 1e-10:.2e} of its bar, sd {e_sd / 1e-10:.2e}")
    assert e_mu < 1e-10 and e_sd < 1e-10, c.name
    for acq in C.ACQS:
        assert torch.equal(out["topk"][acq][0], o2["topk"][acq][0]), (c.name, acq)


PLAIN = C.ONE_TILE + C.GENERAL + C.LOOPED + C.WAVE_PLAN + C.STREAMED + C.BOUNDARY
CHUNKED = {c.name for c in C.LOOPED + C.WAVE_PLAN} | {"str_12_12_looped"}
BOTH_PATHS = {c.name for c in C.STREAMED} | {c.name for c in C.BOUNDARY if C.facts(c)["path"] == 0}


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c.name)
def test_instances_paths_and_loops(case, monkeypatch):
    p = C.problem(case)
    g = build(case, p, monkeypatch)
    Cd = torch.tensor(p.C, device="cuda")
    out = score(g, case, p, Cd)
    check_outputs(case, p, out)
    if C.facts(case)["looped"]:
        check_repeat(g, case, p, out, Cd)
    if case.name in CHUNKED:
        check_looped(g, case, p, out, Cd)
    if case.name in BOTH_PATHS:
        check_other_path(case, p, out, monkeypatch)


@pytest.mark.parametrize("case", [c for c in C.TOPK if c.kind != "refused"], ids=lambda c: c.name)
def test_topk_widths(case, monkeypatch):
    """k = 0 (no top-k buffers are passed: DeviceGP.score hands NULL), 1, 7, 8 across looped
    workgroups; k = 8 over 5 candidates; k = 8 with every value three times."""
    p = C.problem(case)
    g = build(case, p, monkeypatch)
    Cd = torch.tensor(p.C, device="cuda")
    out = score(g, case, p, Cd)
    assert (out["topk"] == {}) == (case.k == 0)
    check_outputs(case, p, out)
    check_repeat(g, case, p, out, Cd)
    if case.kind == "ties3":
        for acq in C.ACQS:
            idx = out["topk"][acq][0].cpu().numpy()
            assert idx[0] < 300 and idx[3] < 300 and idx[6] < 300
            np.testing.assert_array_equal(idx, [idx[0], idx[0] + 300, idx[0] + 600, idx[3], idx[3] + 300,
                                                idx[3] + 600, idx[6], idx[6] + 300], err_msg=acq)


def test_k_past_topk_max_is_refused():
    """k = 9 on a prepared model: the workspace query answers 0 and mpo_gp_acq_score
    MPO_EINVAL with the limit in the message, before any launch."""
    from mpi_opt_amd.gp import DeviceGP

    c = C.by_name("topk_k9")
    p = C.problem(c)
    g = DeviceGP(p.X, p.y, p.st.amp, p.st.length_scale, p.st.noise)
    L = _lib.lib()
    assert L.mpo_gp_score_ws_bytes(ctypes.byref(g.model), c.m, c.k) == 0
    Cd = torch.tensor(p.C, device="cuda")
    with pytest.raises(_lib.MpoError):
        g.score(Cd, p.y_opt, acqs=C.ACQS, k=c.k)
    wsb = L.mpo_gp_score_ws_bytes(ctypes.byref(g.model), c.m, C.TOPK_MAX)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(3 * c.m, dtype=torch.float64, device="cuda")
    tki = torch.full((3 * 16,), -7, dtype=torch.int64, device="cuda")
    rc = L.mpo_gp_acq_score(ctypes.byref(g.model), Cd.data_ptr(), c.m, p.y_opt, 0.01, 1.96, 7, None, None,
                            buf.data_ptr(), c.k, tki.data_ptr(), buf.data_ptr(), ws.data_ptr(), wsb, None)
    assert rc == 1 and b"k=9 outside [0,8]" in L.mpo_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(tki == -7)) and bool(torch.all(buf == 0))      # nothing was launched


@pytest.mark.parametrize("case", C.UNDERFLOW, ids=lambda c: c.name)
def test_underflow_ties(case, monkeypatch):
    """Every EI and PI underflows to +-0: the top-k is 0 .. k-1 (np.argmin's answer,
    through lex_less on -0.0 == 0.0), LCB's is the ordinary one."""
    p = C.problem(case)
    g = build(case, p, monkeypatch)
    Cd = torch.tensor(p.C, device="cuda")
    out = score(g, case, p, Cd)
    check_outputs(case, p, out)
    for acq in ("EI", "PI"):
        v = out["values"][acq].cpu().numpy()
        assert np.all(v == 0.0), acq
        np.testing.assert_array_equal(out["topk"][acq][0].cpu().numpy(), np.arange(case.k), err_msg=acq)
    print(f"SCORE-ZERO {case.name}: EI signs -0: {int(np.count_nonzero(np.signbit(out['values']['EI'].cpu().numpy())))}"
          f" of {len(p.C)}")
    check_repeat(g, case, p, out, Cd)


@pytest.mark.parametrize("case", C.KSTAR, ids=lambda c: c.name)
def test_kstar_range(case, monkeypatch):
    """The Matern over k = 0, 1e-150 .. 1e19: mu within one unit of the np.longdouble
    reference built from the device's own alpha (score_cases.kstar_reference), every
    output finite, sd and the rest at the usual bars."""
    p = C.problem(case)
    g = build(case, p, monkeypatch)
    out = score(g, case, p)
    mu, sd = check_outputs(case, p, out, mu_bar=False)
    st = p.st
    alpha = g.alpha().cpu().numpy()
    np.testing.assert_allclose(alpha, st.alpha, rtol=1e-8, atol=1e-10)
    mu_ref, unit, k = C.kstar_reference(p.X, p.C, st.length_scale, alpha, st.amp, g.y_mean, g.y_std)
    frac = (np.abs(mu.astype(np.longdouble) - mu_ref) / unit).astype(np.float64)
    k0 = k[:, 0]
    parts = [("k <= 30", k0 <= 30), ("30..700", (k0 > 30) & (k0 < 700)), ("700..760", (k0 >= 700) & (k0 <= 760)),
             ("k > 760", k0 > 760)]
    print(f"SCORE-KSTAR {case.name}: largest fraction of a unit {frac.max():.3f} ("
          + ", ".join(f"{name} {frac[sel].max():.3f}" for name, sel in parts) + ")")
    assert np.all(frac <= 1.0), (case.name, float(frac.max()), float(k0[np.argmax(frac)]))
    far = k0 > 800
    assert np.all(mu[far] == mu[far][0])           # K* is exactly 0 there: mu = y_mean, whatever the tile holds
