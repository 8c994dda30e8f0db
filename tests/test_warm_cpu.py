"""remo_warm_t without a GPU: the object cannot be made, and says why; the NULL forms are harmless.  (That the header and
_lib.EXPORTS agree on the new names is tests/test_abi_cpu.py's export test.)"""
import pytest


def _no_device():
    from remo3d_amd import _lib
    L = _lib.load()
    h = L.remo_ctx_create(0)
    if h:
        L.remo_ctx_destroy(h)
    return not h


def test_warm_entries_are_exported():
    from remo3d_amd import _lib
    L = _lib.load()
    names = ["remo_warm_create", "remo_warm_destroy", "remo_warm_clear", "remo_warm_info", "remo_solve_batch_sens_warm", "remo_solve_batch_sens_warm_tensor"]
    assert all(n in _lib.EXPORTS and hasattr(L, n) for n in names)
    assert L.remo_abi_version() == 7


def test_null_forms_are_harmless():
    from remo3d_amd import _lib
    L = _lib.load()
    L.remo_warm_destroy(None)
    L.remo_warm_clear(None)
    assert L.remo_warm_info(None, None, None, None, None) == -1


def test_without_a_device_there_is_no_warm_state():
    """(On a machine with a GPU the same calls make an empty object.)"""
    from remo3d_amd import _lib, solver
    L = _lib.load()
    if _no_device():
        assert not L.remo_warm_create(0)
        assert b"no HIP device" in L.remo_last_error(None)
        with pytest.raises(solver.RemoError, match="no HIP device"):
            solver.WarmState(0)
    else:
        with solver.WarmState(0) as w:
            assert w.info() == dict(n_free=0, n_cols=0, bytes=0, used_last=0)


def test_sweep_cache_has_no_warm_budget_without_a_device():
    from remo3d_amd import inversion
    with inversion.SweepCache() as cache:
        if _no_device():
            assert cache.warm_bytes == 0 and cache.warm_state(0) is None
        else:
            assert cache.warm_bytes > 0
    with inversion.SweepCache(warm=False) as cache:
        assert cache.warm_bytes == 0 and cache.warm_state(0) is None
