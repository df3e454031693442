"""Host side of the isolation building blocks (no GPU): the per-step fp32 retry is opt-in, a result carries no status by default, and
the two new entry points answer a NULL ctx without touching a device."""
import ctypes as C

import numpy as np

from eyoc_amd import _lib
from eyoc_amd import harness as H
from eyoc_amd.registration import RegistrationResult


def test_per_step_fp32_retry_is_opt_in():
    assert H.RegistrationConfig().fp32_retry_per_step is False
    assert RegistrationResult(np.eye(4), 0.0, 0.0).status == 0
    assert H.RETRIED_FP32 != 0 and H.RETRIED_FP32 & (H.RETRIED_FP32 - 1) == 0


def test_new_entry_points_refuse_a_null_ctx():
    lib = _lib.load()
    assert lib.eyoc_registration_accept_degenerate(None, 1) == -1
    dup, rng = (C.c_uint32 * 32)(), (C.c_uint32 * 32)()
    assert lib.eyoc_maps_last_fault_batches(None, dup, rng) == _lib.ERR_INVALID
    assert b"NULL" in lib.eyoc_last_error()
