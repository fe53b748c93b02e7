"""Retiring population members, host side (no GPU): ``mpo_pop_set_active`` /
``mpo_dn_set_active`` before ``bind`` only replan, and ``mpo_*_step_work`` under a
mask equals the work of a plan created from the active members alone."""
import ctypes

import pytest

from mpi_opt_amd import _lib

# (F, k, p, dense): every NT bucket (F 10 / 16 -> 1, 17 -> 2, 33 -> 3, 50 -> 4), k <= 4 (the
# zero-bordered input-gradient list, dgf) and k > 4 (dgrad), and members with >= 3
# weight-gradient m-groups of 512 rows (k^2 F + 1 = 5001 and 1251); batch 10 is not a
# multiple of the 4-sample slab groups
MEMBERS = [(10, 2, 2, 50), (50, 10, 10, 200), (33, 5, 3, 77), (17, 3, 7, 120), (50, 5, 2, 200), (16, 7, 4, 64)]
BATCH = 10
NT1 = [i for i, m in enumerate(MEMBERS) if (m[0] + 15) // 16 == 1]
SMALL_K = [i for i, m in enumerate(MEMBERS) if m[1] <= 4]


def pop_create(members):
    L = _lib.lib()
    arr = (_lib.MpoCnnSpec * len(members))()
    for i, (F, k, p, d) in enumerate(members):
        arr[i] = _lib.MpoCnnSpec(F, k, p, d, 1e-3, 0.25, 7 + i, 0)
    h = ctypes.c_void_p()
    _lib.check(L.mpo_pop_create(arr, len(members), BATCH, ctypes.byref(h)), "mpo_pop_create")
    return h


def work(fn, h):
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(fn(h, ctypes.byref(a), ctypes.byref(b)), "step_work")
    return int(a.value), int(b.value)


def mask_bytes(n, retired):
    return (ctypes.c_uint8 * n)(*[0 if i in retired else 1 for i in range(n)])


def test_mask_sets_cover_what_they_claim():
    assert NT1 == [0, 5] and SMALL_K == [0, 3]


@pytest.mark.parametrize("retired", [[2], NT1, SMALL_K, [0, 2, 5], [1, 2, 3, 4, 5]])
def test_mnist_work_under_a_mask_is_that_of_the_active_members_alone(retired):
    L = _lib.lib()
    h = pop_create(MEMBERS)
    sz0 = _lib.MpoPopSizes()
    _lib.check(L.mpo_pop_sizes(h, ctypes.byref(sz0)))
    full = work(L.mpo_pop_step_work, h)
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(len(MEMBERS), retired), None), "mpo_pop_set_active")
    masked = work(L.mpo_pop_step_work, h)
    fresh_h = pop_create([m for i, m in enumerate(MEMBERS) if i not in retired])
    fresh = work(L.mpo_pop_step_work, fresh_h)
    assert masked == fresh
    assert 0 < masked[0] < full[0] and masked[1] <= full[1]
    # the same mask again is a no-op; the sizes and layouts never move
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(len(MEMBERS), retired), None))
    assert work(L.mpo_pop_step_work, h) == masked
    sz = _lib.MpoPopSizes()
    _lib.check(L.mpo_pop_sizes(h, ctypes.byref(sz)))
    assert (sz.n_params, sz.act_floats, sz.table_bytes, sz.n_members) == (sz0.n_params, sz0.act_floats,
                                                                         sz0.table_bytes, sz0.n_members)
    L.mpo_pop_destroy(fresh_h)
    L.mpo_pop_destroy(h)


def test_mnist_all_retired_then_all_back():
    L = _lib.lib()
    h = pop_create(MEMBERS)
    full = work(L.mpo_pop_step_work, h)
    n = len(MEMBERS)
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(n, range(n)), None))
    assert work(L.mpo_pop_step_work, h) == (0, 0)
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(n, [1]), None))       # any mask may follow any other
    one = work(L.mpo_pop_step_work, h)
    assert 0 < one[0] < full[0]
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(n, []), None))
    assert work(L.mpo_pop_step_work, h) == full
    L.mpo_pop_destroy(h)


def plan_env(monkeypatch, env):
    """The plan knobs are read when a plan is created."""
    monkeypatch.delenv("MPO_POP_PLAN", raising=False)
    monkeypatch.delenv("MPO_POP_PROFILE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def masked_work(members, retired):
    L = _lib.lib()
    h = pop_create(members)
    _lib.check(L.mpo_pop_set_active(h, mask_bytes(len(members), retired), None), "mpo_pop_set_active")
    out = work(L.mpo_pop_step_work, h)
    L.mpo_pop_destroy(h)
    return out


@pytest.mark.parametrize("serial", [{"MPO_POP_PLAN": "streams=1"}, {"MPO_POP_PROFILE": "1"}], ids=["streams1", "profile"])
@pytest.mark.parametrize("retired", [[], [2], [0, 2, 5], [1, 2, 3, 4, 5]])
def test_mnist_serial_step_is_the_same_items_in_one_launch_fewer(monkeypatch, serial, retired):
    """A step on one stream (streams=1, or profiled) reduces both halves of the weight-gradient
    slabs in one launch of twice the grid; with the side stream they are two launches.  The
    walk of mpo_pop_step_work takes the form the real step takes, from the plan alone."""
    plan_env(monkeypatch, {})
    forked = masked_work(MEMBERS, retired)
    plan_env(monkeypatch, serial)
    one_stream = masked_work(MEMBERS, retired)
    assert one_stream[0] == forked[0] > 0
    assert one_stream[1] == forked[1] - 1


def test_mnist_step_work_before_bind_touches_no_device(monkeypatch):
    """mpo_pop_step_work walks the step's own enqueue code under a tally: before bind, with no
    device, it reports what the hand-written count reported (the figures of the parent of the
    tally's introduction for MEMBERS at batch 10) and makes no HIP call -- a launch would fail
    here without a GPU, and an event of the phase timer that cannot be created turns the timer
    off, which mpo_pop_profile would report as MPO_ENOTSUP."""
    L = _lib.lib()
    for env, full, part in [({}, (2596, 41), (1525, 26)),
                            ({"MPO_POP_PLAN": "streams=1"}, (2596, 40), (1525, 25)),
                            ({"MPO_POP_PROFILE": "1"}, (2596, 40), (1525, 25))]:
        plan_env(monkeypatch, env)
        h = pop_create(MEMBERS)
        assert work(L.mpo_pop_step_work, h) == full
        assert work(L.mpo_pop_step_work, h) == full              # a walk leaves the plan as it found it
        _lib.check(L.mpo_pop_set_active(h, mask_bytes(len(MEMBERS), [0, 2, 5]), None), "mpo_pop_set_active")
        assert work(L.mpo_pop_step_work, h) == part
        buf = ctypes.create_string_buffer(256)
        rc = L.mpo_pop_profile(h, buf, len(buf), 0)
        assert buf.value == b""                                  # no phase was ever marked
        assert rc == (0 if "MPO_POP_PROFILE" in env else 3)      # MPO_OK: the timer is still on / MPO_ENOTSUP
        L.mpo_pop_destroy(h)


def dn_create(n, arch=(16, 16, 3, 10, 7, 3, 12, 16), batch=8):
    h = ctypes.c_void_p()
    a = _lib.MpoDnArch(*arch)
    _lib.check(_lib.lib().mpo_dn_create(ctypes.byref(a), n, batch, ctypes.byref(h)), "mpo_dn_create")
    return h


@pytest.mark.parametrize("arch,batch", [((8, 8, 3, 10, 7, 2, 5, 7), 4), ((16, 16, 3, 10, 7, 3, 12, 16), 8)])
def test_densenet_work_shrinks_with_the_active_count(arch, batch):
    L = _lib.lib()
    n = 4
    h = dn_create(n, arch, batch)
    full = work(L.mpo_dn_step_work, h)
    fresh = {}
    for k in (1, 2, 3):
        fh = dn_create(k, arch, batch)
        fresh[k] = work(L.mpo_dn_step_work, fh)
        L.mpo_dn_destroy(fh)
    assert fresh[1][0] < fresh[2][0] < fresh[3][0] < full[0]
    for retired in ([1], [0, 2], [0, 1, 3]):
        _lib.check(L.mpo_dn_set_active(h, mask_bytes(n, retired), None), "mpo_dn_set_active")
        assert work(L.mpo_dn_step_work, h) == fresh[n - len(retired)]
        assert work(L.mpo_dn_step_work, h)[1] == full[1]          # same launches, smaller grids
    _lib.check(L.mpo_dn_set_active(h, mask_bytes(n, range(n)), None))
    assert work(L.mpo_dn_step_work, h) == (0, 0)
    _lib.check(L.mpo_dn_set_active(h, mask_bytes(n, []), None))
    assert work(L.mpo_dn_step_work, h) == full
    sz = _lib.MpoDnSizes()
    _lib.check(L.mpo_dn_sizes(h, ctypes.byref(sz)))
    assert sz.n_members == n
    L.mpo_dn_destroy(h)


def test_null_pointers_are_einval():
    L = _lib.lib()
    h, d = pop_create(MEMBERS[:1]), dn_create(1)
    a = ctypes.c_int64()
    assert L.mpo_pop_set_active(h, None, None) == 1 and b"null" in L.mpo_last_error()
    assert L.mpo_dn_set_active(d, None, None) == 1 and b"null" in L.mpo_last_error()
    assert L.mpo_pop_set_active(None, mask_bytes(1, []), None) == 1
    assert L.mpo_dn_set_active(None, mask_bytes(1, []), None) == 1
    assert L.mpo_pop_step_work(h, None, ctypes.byref(a)) == 1
    assert L.mpo_dn_step_work(d, ctypes.byref(a), None) == 1
    L.mpo_pop_destroy(h)
    L.mpo_dn_destroy(d)
