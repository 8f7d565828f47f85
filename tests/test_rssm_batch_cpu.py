"""icem_rssm_rollout_cost_batch and DeviceRSSMModel.rollout_cost_batch without a GPU: what they refuse before any HIP call
(include/icem_hip.h: a null pointer, n_problems outside [1, 32], a row count < 1, horizon < 1, a bad cost mode ->
ICEM_E_INVALID with a message), and the wrapper's own shape checks.  The pointers handed over here are host addresses
that no accepted call could use: every case must return before the library touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from icem_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.load_library()


def call(lib, rows, horizon=3, mode=0, n_problems=None, null=None):
    """rc of the entry point with dummy (host) buffers; ``null``: the argument passed as NULL."""
    dummy = (C.c_float * 4)()
    ptr = {k: C.c_void_p(C.addressof(dummy)) for k in ("params", "obs0", "actions", "costs")}
    if null in ptr:
        ptr[null] = None
    arr = (C.c_int32 * max(len(rows), 1))(*rows)
    rows_p = None if null == "rows" else arr
    n = len(rows) if n_problems is None else n_problems
    return lib.icem_rssm_rollout_cost_batch(n, rows_p, horizon, mode, ptr["params"], ptr["obs0"], ptr["actions"], ptr["costs"], None)


@pytest.mark.parametrize("null", ["rows", "params", "obs0", "actions", "costs"])
def test_a_null_pointer_is_invalid(lib, null):
    assert call(lib, [4, 5], null=null) == L.ICEM_E_INVALID
    assert b"null" in lib.icem_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(rows=[], n_problems=0), b"n_problems"),
    (dict(rows=[3], n_problems=-1), b"n_problems"),
    (dict(rows=[1] * 33), b"n_problems"),
    (dict(rows=[3, 0]), b"row"),
    (dict(rows=[3, -7, 2]), b"row"),
    (dict(rows=[3, 4], horizon=0), b"horizon"),
    (dict(rows=[3, 4], mode=3), b"cost_mode"),
    (dict(rows=[3, 4], mode=-1), b"cost_mode"),
])
def test_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert call(lib, **kw) == L.ICEM_E_INVALID
    assert word in lib.icem_last_error()


def test_the_wrapper_checks_rows_and_observations_before_the_library():
    """The shape checks come first in rollout_cost_batch and need nothing of the model: an instance without a device."""
    from icem_amd import DeviceRSSMModel
    m = object.__new__(DeviceRSSMModel)
    acts = torch.zeros((5, 3, 6))
    with pytest.raises(ValueError, match="rows sum to 6"):
        m.rollout_cost_batch(np.zeros((2, 230)), acts, [2, 4])
    with pytest.raises(ValueError, match="observations must be"):
        m.rollout_cost_batch(np.zeros((2, 229)), acts, [2, 3])
    with pytest.raises(ValueError, match="observations must be"):
        m.rollout_cost_batch(np.zeros((3, 230)), acts, [2, 3])
    with pytest.raises(ValueError, match="observations must be"):
        m.rollout_cost_batch(np.zeros(230), acts, [5])
    with pytest.raises(ValueError, match="actions must be"):
        m.rollout_cost_batch(np.zeros((1, 230)), torch.zeros((5, 3, 5)), [5])
