"""CPU: the prepared controller's C ABI without a device, and the machine code of its run-time compiled kernels."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dpp_check  # noqa: E402

from lq_mpc_amd import _lib  # noqa: E402


def test_null_arguments():
    L = _lib.lib()
    out = ctypes.c_void_p()
    a = np.zeros(4)
    p = ctypes.c_void_p(a.ctypes.data)
    assert L.lqmpc_controller_create(None, 2, 1, 2, 1, p, p, p, p, p, p, p, None, None, ctypes.byref(out)) == -1
    assert not out.value
    assert L.lqmpc_controller_create_dev(None, 2, 1, 2, 1, p, p, p, p, p, p, p, None, None, ctypes.byref(out)) == -1
    assert L.lqmpc_controller_destroy(None) == 0
    assert L.lqmpc_controller_step(None, p, p, p, None, None) == -1
    assert L.lqmpc_controller_step_dev(None, p, p, p, None, None) == -1
    assert L.lqmpc_controller_reset(None) == -1
    assert L.lqmpc_controller_bytes(None) == 0
    assert L.lqmpc_controller_kernel(None) == b"none"


def test_batch_controller_needs_a_solver_and_a_device():
    from lq_mpc_amd import BatchController, BatchSolver, LqmpcError
    A, B = np.zeros((2, 2, 1)), np.zeros((2, 1, 1))
    args = (3, A, B, np.eye(2), np.eye(1), np.eye(2), [-1.0], [1.0])
    with pytest.raises(LqmpcError):
        BatchController(None, *args)
    if _lib.lib().lqmpc_device_count() == 0:
        with pytest.raises(LqmpcError):
            BatchController(BatchSolver(0), *args)


@pytest.mark.parametrize("shape", [(3, 2, 6), (7, 3, 11)], ids=str)
def test_controller_kernels_compile_without_a_gpu_and_hold_the_dpp_rule(shape, tmp_path):
    L = _lib.lib()
    try:
        assert L.lqmpc_jit_cache_dir(str(tmp_path).encode()) == 0          # an empty cache: the two files that appear are the two kernels
        log = ctypes.create_string_buffer(4096)
        assert L.lqmpc_jit_compile_controller(*shape, log, len(log)) == 2, log.value.decode(errors="replace")
    finally:
        L.lqmpc_jit_cache_dir(_lib.JIT_CACHE.encode())
    objs = sorted(glob.glob(os.path.join(str(tmp_path), "*.hsaco")))
    assert len(objs) == 2
    total = 0
    for o in objs:
        n, bad = dpp_check.check_file(o)
        total += n
        assert not bad, "\n".join(bad[:20])
    # four instances per wavefront: the step broadcasts by DPP (the factor kernel is MFMA and LDS only); one instance per wavefront
    # (n > 32) broadcasts by v_readlane and holds no DPP instruction at all
    assert (total > 0) == (shape[1] * shape[2] <= 32), total
    # outside the 16-lane-row domain: refused, as lqmpc_jit_compile refuses it
    assert L.lqmpc_jit_compile_controller(9, 5, 7, None, 0) == -5
