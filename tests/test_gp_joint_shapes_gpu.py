"""GPU parity of the joint posterior (``mpo_gp_posterior_cov`` / ``mpo_gp_sample``,
``csrc/gp_joint.hip``) over the table of ``tests/joint_cases.py``: every launch-geometry edge
of its four kernels and of ``mpo::blocked_chol`` behind it, up to m = 4096 and n = 2048.

References.  While n, m <= 600 the end-to-end 80-bit chain (``joint_cases.exact_chain``).
Past that each stage is judged against the device output of the stage before it, so the
joint kernels are tested alone and the reference stays cheap:

* covariance and mu from the model's own ``L_inverse()`` and ``alpha()`` lifted to
  ``np.longdouble`` (``posterior_from_factor``); at m = 4096 the fp64 restatement for the whole
  matrix, and one row per 16-row tile row against all columns in 80-bit;
* the factor from one call with Z = I: ``Lc = (samples - mu)^T / y_std``, held to
  ``|A - Lc Lc^T| <= 4 k_blk gamma_{mp+1} |Lc| |Lc^T| + 8 eps amp`` with
  ``A = cov / y_std^2 + jitter amp I`` of the device's own covariance;
* the samples from that Lc and the device's mu in ``np.longdouble``.

Bars: the project's 1e-9 amp y_std^2 on the covariance, exact symmetry, the mu bar of
tests/test_gp_gpu.py, sqrt(diag) within 1e-9 of ``score``'s sd, samples within
1e-9 y_std sqrt(amp); and the derived ``joint_cases.cov_bound`` (ratio <= 1 wherever the
reference is 80-bit).  The argmin is exact wherever the reference's best-to-second gap exceeds
1e-6 of the scale, by value at 1e-9 otherwise, and always ``np.argmin`` of the device's own
samples.  The workspace, and the covariance's outputs, are pre-filled with NaN before every
call: a tile that no wave writes cannot pass on what an earlier call left there.

Every measured figure is printed (``-s`` shows them); DESIGN §4 records a run."""
import ctypes

import numpy as np
import pytest
import torch

from mpi_opt_amd import _lib
from tests import factor_cases as F
from tests import joint_cases as J

pytestmark = pytest.mark.gpu

LD = np.longdouble
MPO_EINVAL, MPO_ENOTSUP = 1, 3


def poison(g, m, s):
    """A fresh NaN-filled joint workspace large enough for (m, s) and (m, 0)."""
    need = max(_lib.lib().mpo_gp_joint_ws_bytes(ctypes.byref(g.model), m, s),
               _lib.lib().mpo_gp_joint_ws_bytes(ctypes.byref(g.model), m, 0))
    assert need > 0
    g._joint_ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=g.device)


_layered = {}


def reference(c, g):
    """The covariance reference of a case: (dict of ``posterior_from_factor``, its kind).  A
    layered one is built once per (n, d, m) and shared, never written: prepare gives the same
    bits for the same inputs, which is asserted on every reuse."""
    if J.is_exact(c):
        return J.exact_chain(c.name), "80-bit chain"
    X, y, C, _ = J.case_inputs(c.name)
    amp, ls, _ = J.theta(c.d)
    torch.cuda.synchronize()
    W, alpha = g.L_inverse().cpu().numpy(), g.alpha().cpu().numpy()
    key = (c.n, c.d, c.m)
    if key in _layered:
        W0, alpha0, r, kind = _layered[key]
        assert np.array_equal(W0, W) and np.array_equal(alpha0, alpha)
        return r, kind
    y_mean, y_std = J.normalise(y)
    if c.m <= J.ROWS_80BIT_MAX:
        r, kind = J.posterior_from_factor(X, C, ls, amp, W, alpha, y_mean, y_std), "80-bit from the device's W"
    else:
        r = J.posterior_from_factor(X, C, ls, amp, W, alpha, y_mean, y_std, t=np.float64)
        r["tile_rows"] = J.posterior_from_factor(X, C, ls, amp, W, alpha, y_mean, y_std, rows=J.tile_rows(c.m))
        kind = "fp64 from the device's W, 80-bit tile rows"
    _layered[key] = (W, alpha, r, kind)
    return r, kind


def run_cov(g, C):
    """``mpo_gp_posterior_cov`` into NaN-filled outputs over a NaN-filled workspace: a tile that
    no wave writes stays NaN whatever the allocator hands out."""
    Ct = g.as_candidates(C)
    m = Ct.shape[0]
    poison(g, m, 0)
    mu = torch.full((m,), float("nan"), dtype=torch.float64, device=g.device)
    cov = torch.full((m, m), float("nan"), dtype=torch.float64, device=g.device)
    _lib.check(_lib.lib().mpo_gp_posterior_cov(ctypes.byref(g.model), Ct.data_ptr(), m, mu.data_ptr(), cov.data_ptr(),
                                               m, g._joint_ws.data_ptr(), g._joint_ws.numel(),
                                               _lib.stream_handle()), "mpo_gp_posterior_cov")
    torch.cuda.synchronize()
    return mu, cov


def check_cov(c, g, r, kind):
    X, y, C, _ = J.case_inputs(c.name)
    C = np.array(C)                                                # a copy: the shared inputs are read-only
    mu_t, cov_t = run_cov(g, C)
    mu, cov = mu_t.cpu().numpy(), cov_t.cpu().numpy()
    if c.m <= J.EXACT_MAX:
        mu_w, cov_w = g.posterior_cov(C)                             # the wrapper: the same bits
        assert torch.equal(mu_w, mu_t) and torch.equal(cov_w, cov_t), c.name
    assert mu.shape == (c.m,) and cov.shape == (c.m, c.m)
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(mu)), c.name
    amp, y_std = r["amp"], r["y_std"]
    assert y_std == g.y_std
    err = np.abs(cov - r["Sn"] * r["Sn"].dtype.type(y_std) ** 2) / y_std ** 2
    e_cov = float(np.max(err)) / amp
    if "tile_rows" in r:
        # the whole matrix against fp64 (the bar), the derived bound on the 80-bit rows only:
        # the fp64 reference carries the very rounding the bound measures
        x = r["tile_rows"]
        rows = x["rows"]
        err_x = np.abs(cov[rows] - x["Sn"] * LD(y_std) ** 2) / y_std ** 2
        e_rows = float(np.max(err_x)) / amp
        ratio = float(np.max(err_x / J.cov_bound(x)))
        assert e_rows <= 1e-9, (c.name, e_rows)
        mu_ref, mu_scale = x["mu"], x["mu_scale"]
    else:
        ratio = float(np.max(err / J.cov_bound(r)))
        mu_ref, mu_scale = r["mu"], r["mu_scale"]
    e_mu = float(np.max(np.abs(mu - mu_ref) / mu_scale))
    sd = g.score(C, float(np.min(y)), acqs=("EI",))["sd"].cpu().numpy()
    e_sd = float(np.max(np.abs(np.sqrt(np.maximum(np.diag(cov), 0.0)) - sd) / sd))
    print(f"JOINT-COV {c.name} [n {c.n} d {c.d} m {c.m}; v_grid {J.v_grid(c.n, c.m)}, cov_trips {J.cov_trips(c.m)} "
          f"({J.cov_last_trip_waves(c.m)} waves on the last); {kind}]: cov {e_cov:.3e} of amp y_std^2"
          + (f" (80-bit tile rows {e_rows:.3e})" if "tile_rows" in r else "")
          + f", {ratio:.3e} of the derived bound, mu {e_mu:.3e}, sqrt(diag) vs sd {e_sd:.3e}")
    assert np.array_equal(cov, cov.T), c.name
    assert e_cov <= 1e-9, (c.name, e_cov)
    assert ratio <= 1.0, (c.name, ratio)
    assert e_mu < 1e-9, (c.name, e_mu)
    assert e_sd <= 1e-9, (c.name, e_sd)
    return mu, cov


def check_samples(c, g, r, mu, cov):
    X, y, C, Z = (np.array(a) for a in J.case_inputs(c.name))
    amp, y_std = r["amp"], r["y_std"]
    scale = y_std * np.sqrt(amp)
    exact = J.is_exact(c)
    # the factor: Z = I, s = m
    poison(g, c.m, max(c.m, c.s))
    out = g.sample(C, np.eye(c.m), jitter=J.JITTER)
    assert out["info"] == 0, (c.name, out["info"])
    S_i = out["samples"].cpu().numpy()
    assert np.all(np.isfinite(S_i)), c.name
    Lc = (S_i - mu[None, :]).T / y_std
    del S_i, out
    assert np.all(np.triu(Lc, 1) == 0), c.name
    A = cov / y_std ** 2 + J.JITTER * amp * np.eye(c.m)
    ratio, k_blk, res = J.factor_ratio(A, Lc, amp, exact_product=exact)
    # the samples and the argmin of the case's Z
    poison(g, c.m, max(c.m, c.s))
    out = g.sample(C, Z, jitter=J.JITTER)
    assert out["info"] == 0, (c.name, out["info"])
    S, am = out["samples"].cpu().numpy(), out["argmin"].cpu().numpy()
    assert S.shape == (c.s, c.m) and am.shape == (c.s,) and am.dtype == np.int64
    if exact:
        S_ref = r["S"]
        e_l = float(np.max(np.abs(Lc - r["Lc"]))) / np.sqrt(amp)
    else:
        S_ref = mu.astype(LD)[None, :] + LD(y_std) * (Lc.astype(LD) @ Z.astype(LD)).T
        e_l = float("nan")
    e_s = float(np.max(np.abs(S - S_ref))) / scale
    ok, by_value = J.argmin_check(S_ref, am, scale)
    mp = J.joint_mp(c.m)
    print(f"JOINT-SAMPLE {c.name} [m {c.m} s {c.s}; mp {mp}, factored-matrix cov_trips {J.cov_trips(mp)}, "
          f"chol_update_trips {J.chol_update_trips(mp)}, sample_grid {J.sample_grid(c.m, c.s)}, idle waves "
          f"{J.sample_idle_waves(c.m)}, argmin_blocks {J.argmin_blocks(c.s)}; {'80-bit chain' if exact else 'layered'}]: "
          f"factor residual {res / amp:.3e} of amp, {ratio:.3e} of its bound (k_blk {k_blk:.1f}), Lc vs exact "
          f"{e_l:.3e} of sqrt(amp), samples {e_s:.3e} of y_std sqrt(amp), {by_value} draws judged by value, "
          f"{len(set(am.tolist()))} distinct argmins")
    assert ratio <= 1.0, (c.name, ratio)
    assert e_s <= 1e-9, (c.name, e_s)
    assert by_value <= 1, (c.name, by_value)
    assert np.all(ok), (c.name, np.flatnonzero(~ok)[:8])
    assert np.array_equal(am, np.argmin(S, axis=1)), c.name       # np.argmin of the device's own samples


@pytest.mark.parametrize("case", J.CASES, ids=lambda c: c.name)
def test_joint_case(case):
    X, y, C, _ = J.case_inputs(case.name)
    g = J.device_gp(np.array(X), np.array(y), case.d)              # copies: the shared inputs are read-only
    r, kind = reference(case, g)
    mu, cov = check_cov(case, g, r, kind)
    if case.what == "sample":
        check_samples(case, g, r, mu, cov)


# ---- argmin placement and ties ---------------------------------------------------------------
@pytest.fixture(scope="module")
def placement_gp():
    X, y, _, _, _ = J.placement_pool()
    return J.device_gp(np.array(X), np.array(y), J.PLACE_D)


def placed(g, C, s):
    poison(g, J.PLACE_M, s)
    out = g.sample(C, np.zeros((J.PLACE_M, s)), jitter=J.PLACE_JITTER)
    assert out["info"] == 0
    S, am = out["samples"].cpu().numpy(), out["argmin"].cpu().numpy()
    assert np.all(np.isfinite(S))
    return S, am


@pytest.mark.parametrize("i", J.PLACE_SINGLE)
def test_argmin_follows_the_minimum_to_every_boundary(placement_gp, i):
    """Z = 0: every draw is mu, and its argmin is wherever the candidate of lowest mu is put
    -- the first and last row of a q, a lane group, a wave and a workgroup."""
    S, am = placed(placement_gp, J.placement_candidates(i), 1)
    assert am.tolist() == [i] and int(np.argmin(S[0])) == i


@pytest.mark.parametrize("i1,i2,why", J.PLACE_DUP, ids=[f"{a}_{b}" for a, b, _ in J.PLACE_DUP])
def test_argmin_tie_goes_to_the_lowest_index(placement_gp, i1, i2, why):
    """Two copies of that candidate: bit-equal samples (the premise), the lower index wins at
    whichever of ``lex_less``'s five levels the two meet."""
    C = J.placement_candidates(i1, i2)
    for s in (1, J.PLACE_S):
        S, am = placed(placement_gp, C, s)
        assert S[:, i1].tobytes() == S[:, i2].tobytes(), (i1, i2, why)
        assert np.all(np.argmin(S, axis=1) == i1)
        assert am.tolist() == [i1] * s, (i1, i2, why, am)


# ---- failure reporting past the first block --------------------------------------------------
@pytest.mark.parametrize("second", (False, True))
def test_failed_factor_past_the_first_block(second):
    """The observation itself as query 40 (block 1, column 8): info = 41, also with a copy of
    it at 45 -- the first failure wins."""
    from mpi_opt_amd.gp import DeviceGP

    X, y, ls, Q = J.failure_inputs(second)
    g = DeviceGP(X, y, F.PIVOT_AMP, ls, -1.0)
    var = np.diag(g.posterior_cov(Q)[1].cpu().numpy())
    bad = [J.FAIL_AT, J.FAIL_AGAIN] if second else [J.FAIL_AT]
    assert np.all(var[bad] < -1.0) and np.all(np.delete(var, bad) > 1.0)
    poison(g, 70, 2)
    assert g.sample(Q, np.random.RandomState(3).standard_normal((70, 2)), jitter=J.JITTER)["info"] == J.FAIL_AT + 1


# ---- the C ABI --------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.int64)


class Abi:
    """``lib()`` called directly on the model of ``ABI_CASE``: every output pre-filled with the
    sentinel, the workspace with NaN bytes and followed by a guard band."""

    def __init__(self):
        n, d, m, s = J.ABI_CASE
        X, y, C, Z = J.inputs(n, d, m, s)
        self.g = J.device_gp(X, y, d)
        self.m, self.s, self.C, self.Z = m, s, dev(C), dev(Z)
        self.L = _lib.lib()
        self.need = {k: self.L.mpo_gp_joint_ws_bytes(ctypes.byref(self.g.model), m, k) for k in (0, s)}
        assert 0 < self.need[0] < self.need[s]

    def ws(self, k):
        return torch.full((self.need[k] + J.GUARD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")

    def guard_intact(self, ws, k):
        torch.cuda.synchronize()
        return bool(torch.all(ws[self.need[k]:] == 0xA5))

    def cov(self, ldc=None, want_mu=True, ws_bytes=None):
        m = self.m
        ldc = m if ldc is None else ldc
        mu = torch.full((m,), F.SENTINEL, dtype=torch.float64, device="cuda")
        cov = torch.full((m, ldc), F.SENTINEL, dtype=torch.float64, device="cuda")
        ws = self.ws(0)
        rc = self.L.mpo_gp_posterior_cov(ctypes.byref(self.g.model), self.C.data_ptr(), m,
                                         mu.data_ptr() if want_mu else None, cov.data_ptr(), ldc, ws.data_ptr(),
                                         self.need[0] if ws_bytes is None else ws_bytes, _lib.stream_handle())
        ok = self.guard_intact(ws, 0)
        return rc, mu, cov, ok

    def sample(self, want_samples=True, want_argmin=True, ws_bytes=None):
        m, s = self.m, self.s
        S = torch.full((s, m), F.SENTINEL, dtype=torch.float64, device="cuda")
        am = torch.full((s,), -9, dtype=torch.int64, device="cuda")
        info = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        ws = self.ws(s)
        rc = self.L.mpo_gp_sample(ctypes.byref(self.g.model), self.C.data_ptr(), m, self.Z.data_ptr(), s, J.JITTER,
                                  S.data_ptr() if want_samples else None, am.data_ptr() if want_argmin else None,
                                  info.data_ptr(), ws.data_ptr(), self.need[s] if ws_bytes is None else ws_bytes,
                                  _lib.stream_handle())
        ok = self.guard_intact(ws, s)
        return rc, S, am, int(info.item()), ok


@pytest.fixture(scope="module")
def abi():
    return Abi()


def test_abi_ldc_null_mu_and_the_workspace_extent(abi):
    m = abi.m
    rc, mu, cov, ok = abi.cov()
    assert rc == 0 and ok
    assert bool(torch.all(cov != F.SENTINEL)) and bool(torch.all(mu != F.SENTINEL))
    # the wrapper's result (a workspace of its own, no guard band) is these bits
    mu_w, cov_w = abi.g.posterior_cov(abi.C)
    assert torch.equal(mu_w, mu) and torch.equal(cov_w, cov)
    rc, mu2, wide, ok = abi.cov(ldc=m + J.ABI_PAD)
    assert rc == 0 and ok and torch.equal(mu2, mu)
    assert np.array_equal(bits(wide[:, :m].contiguous()), bits(cov))
    assert bool(torch.all(wide[:, m:] == F.SENTINEL))
    rc, mu3, cov3, ok = abi.cov(want_mu=False)
    assert rc == 0 and ok and np.array_equal(bits(cov3), bits(cov)) and bool(torch.all(mu3 == F.SENTINEL))
    rc, mu4, cov4, ok = abi.cov(ws_bytes=abi.need[0] - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in abi.L.mpo_last_error()
    assert ok and bool(torch.all(cov4 == F.SENTINEL)) and bool(torch.all(mu4 == F.SENTINEL))      # nothing was launched


def test_abi_null_outputs_and_the_workspace_extent(abi):
    rc, S, am, info, ok = abi.sample()
    assert rc == 0 and info == 0 and ok
    assert bool(torch.all(S != F.SENTINEL)) and bool(torch.all((am >= 0) & (am < abi.m)))
    w = abi.g.sample(abi.C, abi.Z, jitter=J.JITTER)
    assert torch.equal(w["samples"], S) and torch.equal(w["argmin"], am) and w["info"] == 0
    rc, S2, am2, info2, ok = abi.sample(want_samples=False)
    assert rc == 0 and info2 == 0 and ok and torch.equal(am2, am) and bool(torch.all(S2 == F.SENTINEL))
    rc, S3, am3, info3, ok = abi.sample(want_argmin=False)
    assert rc == 0 and info3 == 0 and ok and np.array_equal(bits(S3), bits(S)) and bool(torch.all(am3 == -9))
    rc, S4, am4, info4, ok = abi.sample(want_samples=False, want_argmin=False)
    assert rc == 0 and info4 == 0 and ok                            # info is still written
    assert bool(torch.all(S4 == F.SENTINEL)) and bool(torch.all(am4 == -9))
    rc, S5, am5, info5, ok = abi.sample(ws_bytes=abi.need[abi.s] - 1)
    assert rc == MPO_EINVAL and b"workspace too small" in abi.L.mpo_last_error()
    assert ok and info5 == -9 and bool(torch.all(S5 == F.SENTINEL)) and bool(torch.all(am5 == -9))


def test_more_than_smax_draws_are_refused_before_any_launch(abi):
    """s = MPO_JOINT_SMAX + 1 at m = 1: ``MPO_ENOTSUP`` from the host checks, no workspace size,
    a ``ValueError`` from the wrapper; nothing is written.  The accepted maximum is the table's
    last case."""
    assert J.CASES[-1].s == _lib.MPO_JOINT_SMAX == J.JOINT_SMAX and J.CASES[-1].m == 1
    s = J.JOINT_SMAX + 1
    md = ctypes.byref(abi.g.model)
    assert abi.L.mpo_gp_joint_ws_bytes(md, 1, s) == 0 and abi.L.mpo_gp_joint_ws_bytes(md, 1, s - 1) > 0
    S = torch.full((16,), F.SENTINEL, dtype=torch.float64, device="cuda")
    am = torch.full((16,), -9, dtype=torch.int64, device="cuda")
    info = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    ws = abi.ws(abi.s)
    rc = abi.L.mpo_gp_sample(md, abi.C.data_ptr(), 1, abi.Z.data_ptr(), s, J.JITTER, S.data_ptr(), am.data_ptr(),
                             info.data_ptr(), ws.data_ptr(), 1 << 40, _lib.stream_handle())
    assert rc == MPO_ENOTSUP and b"s=1048561 outside the supported s <= 1048560" in abi.L.mpo_last_error()
    torch.cuda.synchronize()
    assert int(info.item()) == -9 and bool(torch.all(S == F.SENTINEL)) and bool(torch.all(am == -9))
    assert bool(torch.all(ws == 0xA5))
    with pytest.raises(ValueError, match="at most 1048560"):
        abi.g.sample(abi.C[:1], torch.zeros(1, s, dtype=torch.float64, device="cuda"))
