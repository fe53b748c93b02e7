"""Host-side dispatch of the two GP scoring paths (no GPU): ``mpo_gp_score_path``
and the workspace queries on host structs -- the LDS boundary per padded width,
the MPO_GP_SCORE / MPO_GP_PANEL switches and the n = 2048 limit."""
import ctypes

import pytest

from mpi_opt_amd import _lib

PAD = {4: 4, 8: 8, 10: 12, 12: 12, 16: 16, 32: 32}
MIB = 1 << 20


def model(n, d):
    return _lib.MpoGpModel(n=n, d=d, dp=PAD[d], np16=(n + 15) // 16 * 16)


def path(n, d):
    return _lib.lib().mpo_gp_score_path(ctypes.byref(model(n, d)))


def score_ws(n, d, m=200, k=5):
    return _lib.lib().mpo_gp_score_ws_bytes(ctypes.byref(model(n, d)), m, k)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("MPO_GP_SCORE", raising=False)
    monkeypatch.delenv("MPO_GP_PANEL", raising=False)


# the last np16 whose K* tile (16 candidates x np16 observations) fits the 160 KiB LDS
@pytest.mark.parametrize("d,last", [(4, 1248), (8, 1232), (12, 1232), (32, 1216)])
def test_path_boundary_per_padded_width(d, last):
    assert path(last, d) == 0
    assert path(last - 15, d) == 0          # same np16
    assert path(last + 1, d) == 1
    assert path(2048, d) == 1
    assert path(1, d) == 0
    assert 0 < score_ws(last, d) <= score_ws(last + 1, d)   # one panel may still hold all of K*: no partial rows
    assert _lib.lib().mpo_gp_prepare_ws_bytes(last + 1, d) > 0


def test_d10_boundary_matches_gpu_dispatch_test():
    assert path(1232, 10) == 0 and path(1233, 10) == 1


def test_limit_is_2048():
    L = _lib.lib()
    assert L.mpo_gp_prepare_ws_bytes(2048, 10) > 2 * 2048 * 2048 * 8
    assert L.mpo_gp_prepare_ws_bytes(2049, 10) == 0
    assert L.mpo_gp_prepare_ws_bytes(2048, 33) == 0
    assert score_ws(2048, 10, m=1_000_000) > 0
    assert score_ws(2049, 10) == 0
    assert path(2049, 10) < 0
    assert path(0, 10) < 0
    assert L.mpo_gp_score_path(None) < 0
    assert L.mpo_gp_score_path(ctypes.byref(_lib.MpoGpModel(n=100, d=10, dp=10, np16=112))) < 0   # dp never 10
    assert L.mpo_gp_score_path(ctypes.byref(_lib.MpoGpModel(n=100, d=10, dp=12, np16=100))) < 0   # np16 not padded


def test_n_2049_is_not_supported_and_the_message_names_the_limit():
    """The entry points refuse before any device call: no GPU is needed to see it."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    m = _lib.MpoGpModel()
    assert L.mpo_gp_prepare(p, p, 2049, 10, p, 1.0, 0.1, 0.0, 1.0, ctypes.byref(m), p, 64, None) == 3   # MPO_ENOTSUP
    assert b"2048" in L.mpo_last_error()
    big = model(2049, 10)
    assert L.mpo_gp_acq_score(ctypes.byref(big), p, 16, 0.0, 0.01, 1.96, 1, p, p, p, 0, None, None, p, 64, None) == 3
    assert b"2048" in L.mpo_last_error()
    assert L.mpo_gp_ei_score(ctypes.byref(big), p, 16, 0.0, 0.01, p, p, p, p, p, 64, None) == 3
    assert b"2048" in L.mpo_last_error()


def test_streamed_workspace_growth_is_bounded():
    """The partial rows of the later panels: 256 workgroups x 51 column tiles x 2 KiB
    at n = 2048, d = 10 with the default panel; never above 48 MiB + the resident size,
    whatever panel is forced."""
    resident_like = score_ws(1232, 10, m=1_000_000)
    grown = score_ws(2048, 10, m=1_000_000) - resident_like
    assert 0 < grown <= 26 * MIB
    assert score_ws(2048, 32, m=1_000_000) - resident_like <= 27 * MIB


def test_env_switches(monkeypatch):
    monkeypatch.setenv("MPO_GP_SCORE", "streamed")
    assert path(57, 4) == 1 and path(1, 4) == 1 and path(2049, 10) < 0
    base = score_ws(300, 16, m=1_000_000)
    monkeypatch.setenv("MPO_GP_PANEL", "16")
    assert path(57, 4) == 1
    small_panel = score_ws(300, 16, m=1_000_000)
    assert small_panel > base                       # a single panel keeps no partial rows
    assert small_panel - base <= 49 * MIB
    monkeypatch.setenv("MPO_GP_PANEL", "64")
    assert path(300, 16) == 1 and score_ws(300, 16) > 0
    monkeypatch.setenv("MPO_GP_PANEL", "4096")      # larger than fits: clamped, not refused
    assert path(2048, 10) == 1 and score_ws(2048, 10) > 0
    for bad in ("24", "8", "0", "-16", "16x", "abc"):
        monkeypatch.setenv("MPO_GP_PANEL", bad)
        assert path(57, 4) < 0, bad
        assert score_ws(57, 4) == 0, bad
    monkeypatch.setenv("MPO_GP_SCORE", "resident")  # the automatic choice: the panel plays no part below the limit
    assert path(57, 4) == 0 and score_ws(57, 4) > 0
    assert path(1233, 10) < 0                       # ... but does past it
    monkeypatch.setenv("MPO_GP_PANEL", "32")
    assert path(1232, 10) == 0 and path(1233, 10) == 1
    monkeypatch.setenv("MPO_GP_SCORE", "something-else")
    assert path(1232, 10) == 0 and path(1233, 10) == 1


def test_optimizer_refuses_more_than_2048_points_before_any_device_work():
    """No GPU here: the ValueError must come before the refit touches a device."""
    from mpi_opt_amd.optimizer import Optimizer

    opt = Optimizer([(0.0, 1.0), (0.0, 1.0)], acq_func="EI", random_state=0, n_initial_points=4000)
    pts = [[i / 4000.0, 0.5] for i in range(2040)]
    opt.tell(pts, [p[0] for p in pts])              # still inside the initial points: no GP
    opt._n_initial_points = 0
    with pytest.raises(ValueError, match=r"2048.*lies"):
        opt.tell([[0.1, 0.2]] * 9, [0.0] * 9)       # n = 2049
    assert len(opt.yi) == 2040                      # nothing was taken
    with pytest.raises(ValueError, match=r"2048.*lies"):
        opt.ask(9)                                  # 2040 told + 9 lies
