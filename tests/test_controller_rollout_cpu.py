"""No GPU: the C ABI and the Python surface of the prepared controller's rollout (lqmpc_controller_rollout*, BatchController.rollout)."""
import ctypes
import os
import re

import pytest

from lq_mpc_amd import BatchController, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqmpc_controller_rollout", "lqmpc_controller_rollout_dev", "lqmpc_jit_compile_controller_rollout")


def header():
    return open(os.path.join(ROOT, "include", "lqmpc.h")).read()


def test_header_declares_and_library_exports_the_new_symbols():
    h = header()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, h, re.M), name
        assert name in _lib.EXPORTS
        getattr(L, name)
    assert re.search(r"int lqmpc_controller_rollout\(lqmpc_controller \*c, int T, const double \*x0,\s*const double \*A_true, "
                     r"const double \*B_true, int true_per_instance,\s*double \*JT, double \*X, double \*U, int32_t \*status, "
                     r"int32_t \*iters\);", h)


def test_options_struct_is_unchanged():
    # 2 x uint32, 3 x double, 12 x int32 (include/lqmpc.h): the rollout adds no option
    assert ctypes.sizeof(_lib.Options) == 2 * 4 + 3 * 8 + 12 * 4 == 80
    o = _lib.Options()
    _lib.lib().lqmpc_default_options(ctypes.byref(o))
    assert o.struct_size == 80


def test_bad_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (L.lqmpc_controller_rollout, L.lqmpc_controller_rollout_dev):
        assert fn(None, 3, p, p, p, 0, p, None, None, None, None) == -1            # no controller
        assert fn(None, 0, p, p, p, 0, p, None, None, None, None) == -1            # T = 0
        assert fn(None, 3, None, p, p, 0, p, None, None, None, None) == -1
        assert fn(None, 3, p, None, p, 0, p, None, None, None, None) == -1
        assert fn(None, 3, p, p, None, 1, p, None, None, None, None) == -1
        assert fn(None, 3, p, p, p, 0, None, None, None, None, None) == -1
        assert L.lqmpc_last_error()


def test_python_surface():
    assert callable(BatchController.rollout) and callable(BatchController.rollout_dev)


def test_run_time_compile_of_the_rollout_kernel(tmp_path):
    L = _lib.lib()
    assert L.lqmpc_jit_cache_dir(str(tmp_path).encode()) == 0
    try:
        assert _lib.jit_compile_controller(3, 2, 6) == 2                          # pinned by the existing tests: stays 2
        assert _lib.jit_compile_controller_rollout(3, 2, 6) == 1
        assert _lib.jit_compile_controller_rollout(7, 3, 11) == 1
        log = ctypes.create_string_buffer(256)
        assert L.lqmpc_jit_compile_controller_rollout(9, 5, 7, log, len(log)) == -5
        with pytest.raises(_lib.LqmpcError):
            _lib.jit_compile_controller_rollout(9, 5, 7)
    finally:
        assert L.lqmpc_jit_cache_dir(_lib.JIT_CACHE.encode()) == 0
